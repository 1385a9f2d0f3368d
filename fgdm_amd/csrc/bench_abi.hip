// Micro-benchmark entries of the C ABI (fgdm_bench_*): one kernel family each on random operands of their own, timed with HIP
// events on the null stream.  No engine (tools/bench_*.py call them).
#include "engine_shared.h"
#include "knobs.h"

// FGDM_BENCH_DATA_SCALE (default 1, read at every call) scales the random operands: 0 gives the all-zero run, and the gap to random
// data is the chip lowering its clock under load (data-dependent power draw against instruction issue)
static float data_scale() { return (float)atof(knob_text(KNOB_BENCH_DATA_SCALE)); }

// *avg_ms = average device milliseconds of `run()` over `iters` calls, after `warm` calls that are not timed
template <class Run>
static int time_launches(int warm, int iters, float* avg_ms, Run&& run) {
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0)); HIP_TRY(hipEventCreate(&e1));
    int rc = FGDM_OK;
    for (int i = 0; i < warm && rc == FGDM_OK; ++i) rc = run();
    HIP_TRY(hipEventRecord(e0, nullptr));
    for (int i = 0; i < iters && rc == FGDM_OK; ++i) rc = run();
    HIP_TRY(hipEventRecord(e1, nullptr));
    HIP_TRY(hipEventSynchronize(e1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    *avg_ms = ms / iters;
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return rc;
}

extern "C" {

// Micro-benchmark of one conv / linear shape on random data: average device ms over `iters` launches.
int fgdm_bench_igemm(int B, int H, int W, int C0, int C1, int Cout, int ksize, int stride, int upsample, int act,
                     int use_resid, int cfg, int iters, float* avg_ms) {
    if (!avg_ms || iters <= 0 || (ksize != 1 && ksize != 3)) return FGDM_ERR_ARG;
    const int Cin = C0 + C1, taps = ksize * ksize, K = taps * Cin;
    if (Cin & 63) return FGDM_ERR_ARG;
    int Ho = H, Wo = W, mode = ksize == 3 ? IG_CONV3 : IG_LINEAR;
    if (ksize == 3 && upsample) { Ho = 2 * H; Wo = 2 * W; mode = IG_CONV3_UP2; }
    else if (ksize == 3 && stride == 2) { Ho = (H - 1) / 2 + 1; Wo = (W - 1) / 2 + 1; mode = IG_CONV3_S2; }
    const size_t M = (size_t)B * Ho * Wo, nin = (size_t)B * H * W;
    const size_t npad = igemm_npad(Cout);
    const int nout = act == ACT_GEGLU ? Cout / 2 : Cout;
    unsigned st = 12345u;
    const float dscale = data_scale();
    auto rnd = [&]() { st = st * 1664525u + 1013904223u; return dscale * (((st >> 9) & 0xffff) / 32768.0f - 1.0f); };
    std::vector<half_t> hx0(nin * C0), hx1(nin * (size_t)std::max(C1, 1)), hw(npad * (size_t)K), hr(M * nout);
    std::vector<float> hb(npad);
    for (auto& v : hx0) v = (half_t)rnd();
    for (auto& v : hx1) v = (half_t)rnd();
    const float ws = 1.0f / sqrtf((float)K);
    for (auto& v : hw) v = (half_t)(rnd() * ws);
    for (auto& v : hr) v = (half_t)rnd();
    for (auto& v : hb) v = rnd() * 0.1f;
    TmpDev tmp;
    half_t* out = tmp.alloc<half_t>(M * nout);
    if (!out) return FGDM_ERR_NOMEM;
    IgemmArgs a{};
    a.A0 = tmp.up(hx0); a.C0 = C0; a.A1 = C1 ? tmp.up(hx1) : nullptr; a.C1 = C1;
    a.Wt = tmp.up(hw); a.bias = tmp.up(hb); a.zero = g_zero_page();
    a.resid = use_resid ? tmp.up(hr) : nullptr; a.ld_res = nout;
    if (!a.A0 || !a.Wt || !a.bias || !a.zero) return FGDM_ERR_NOMEM;
    a.B = B; a.H = H; a.W = W; a.Ho = Ho; a.Wo = Wo; a.mode = mode;
    a.M = (int)M; a.N = Cout; a.K = K; a.act = act; a.out_kind = OUT_F16; a.out = out; a.ld_out = nout;
    a.rows_per_sample = Ho * Wo; a.scale = 1.f; a.force_cfg = cfg & 0xff; a.debug = (cfg >> 8) & 0xff;
    if (igemm_up_phase(a)) {        // the engine's dispatch: four 2x2 phase GEMMs in one launch, on random phase kernels [4][npad][4 C]
        std::vector<half_t> hp(4 * npad * (size_t)(4 * Cin));
        const float ps = 1.0f / sqrtf(2.25f * Cin);       // a phase tap sums 1 / 2 / 4 of the 3x3 taps: 2.25 on average
        for (auto& v : hp) v = (half_t)(rnd() * ps * 3.0f);
        const half_t* wph = tmp.up(hp);
        if (!wph) return FGDM_ERR_NOMEM;
        a = igemm_phase_args(a, wph);
    }
    if ((cfg & 0xff) == 0 && plan_splitk(a, tmp) != FGDM_OK) return FGDM_ERR_NOMEM;
    return time_launches(3, iters, avg_ms, [&]() { return igemm_launch(a, nullptr); });
}

// Feed-forward pair of a transformer block (GEGLU projection C -> 8C, then 4C -> C with the residual) on M random token rows,
// evaluated in row chunks of `chunk` rows that reuse ONE intermediate buffer: does the 4C intermediate of a chunk stay on chip
// (L2 / Infinity Cache) between its producer and its consumer?  chunk = M: the two launches the engine makes today.
int fgdm_bench_ff(int M, int Cw, int chunk, int iters, float* avg_ms) {
    if (!avg_ms || iters <= 0 || M <= 0 || chunk <= 0 || (Cw % 320) || (M % chunk)) return FGDM_ERR_ARG;
    const int N1 = 8 * Cw, K2 = 4 * Cw;
    unsigned st = 4321u;
    auto rnd = [&]() { st = st * 1664525u + 1013904223u; return ((st >> 9) & 0xffff) / 32768.0f - 1.0f; };
    std::vector<half_t> hx((size_t)M * Cw), hw1(igemm_npad(N1) * (size_t)Cw), hw2(igemm_npad(Cw) * (size_t)K2);
    std::vector<float> hb1(igemm_npad(N1)), hb2(igemm_npad(Cw));
    for (auto& v : hx) v = (half_t)rnd();
    for (auto& v : hw1) v = (half_t)(rnd() / sqrtf((float)Cw));
    for (auto& v : hw2) v = (half_t)(rnd() / sqrtf((float)K2));
    for (auto& v : hb1) v = rnd() * 0.1f;
    for (auto& v : hb2) v = rnd() * 0.1f;
    TmpDev tmp;
    half_t *h = tmp.alloc<half_t>((size_t)chunk * K2), *out = tmp.alloc<half_t>((size_t)M * Cw);
    if (!h || !out) return FGDM_ERR_NOMEM;
    const half_t* x = tmp.up(hx);
    IgemmArgs g{}, f{};
    g.Wt = tmp.up(hw1); g.bias = tmp.up(hb1); g.zero = g_zero_page();
    f.Wt = tmp.up(hw2); f.bias = tmp.up(hb2); f.zero = g.zero;
    if (!x || !g.Wt || !g.bias || !f.Wt || !f.bias || !g.zero) return FGDM_ERR_NOMEM;
    g.C0 = Cw; g.B = 1; g.H = 1; g.W = chunk; g.Ho = 1; g.Wo = chunk; g.M = chunk; g.N = N1; g.K = Cw; g.mode = IG_LINEAR;
    g.act = ACT_GEGLU; g.out_kind = OUT_F16; g.out = h; g.ld_out = K2; g.rows_per_sample = chunk; g.scale = 1.f;
    f.A0 = h; f.C0 = K2; f.B = 1; f.H = 1; f.W = chunk; f.Ho = 1; f.Wo = chunk; f.M = chunk; f.N = Cw; f.K = K2; f.mode = IG_LINEAR;
    f.act = ACT_NONE; f.out_kind = OUT_F16; f.ld_out = Cw; f.ld_res = Cw; f.rows_per_sample = chunk; f.scale = 1.f;
    auto pass = [&]() {
        int rc = FGDM_OK;
        for (int r0 = 0; r0 < M && rc == FGDM_OK; r0 += chunk) {
            g.A0 = x + (size_t)r0 * Cw;
            rc = igemm_launch(g, nullptr);
            f.resid = x + (size_t)r0 * Cw; f.out = out + (size_t)r0 * Cw;
            if (rc == FGDM_OK) rc = igemm_launch(f, nullptr);
        }
        return rc;
    };
    return time_launches(2, iters, avg_ms, pass);
}

// Micro-benchmark of the fused attention kernel on random data: average device ms over `iters` launches.
// capture 0: attention_launch; 1: the capturing instantiation alone (per-head planes written); 2: ... and the head reduction
static int bench_attention(int B, int heads, int T, int Tk, int d, int capture, int iters, float* avg_ms) {
    if (!avg_ms || iters <= 0 || B <= 0 || heads <= 0 || T <= 0 || Tk <= 0) return FGDM_ERR_ARG;
    const int C = heads * d, Tkp = (Tk + 63) / 64 * 64;
    unsigned st = 4242u;
    auto rnd = [&]() { st = st * 1664525u + 1013904223u; return ((st >> 9) & 0xffff) / 32768.0f - 1.0f; };
    std::vector<half_t> hq((size_t)B * T * C), hk((size_t)B * Tk * C), hv((size_t)B * C * Tkp, (half_t)0);
    const float ds = data_scale();
    for (auto& v : hq) v = (half_t)(rnd() * 1.5f * ds);
    for (auto& v : hk) v = (half_t)(rnd() * 1.5f * ds);
    for (size_t r = 0; r < (size_t)B * C; ++r) for (int t = 0; t < Tk; ++t) hv[r * Tkp + t] = (half_t)(rnd() * ds);
    TmpDev tmp;
    half_t* o = tmp.alloc<half_t>((size_t)B * T * C);
    if (!o) return FGDM_ERR_NOMEM;
    const half_t *dq = tmp.up(hq), *dk = tmp.up(hk), *dv = tmp.up(hv);
    if (!dq || !dk || !dv) return FGDM_ERR_NOMEM;
    if (!capture) return time_launches(3, iters, avg_ms, [&]() { return attention_launch(dq, C, dk, C, dv, Tkp, o, C, B, heads, T, Tk, d, 0, nullptr); });
    float* planes = tmp.alloc<float>(attention_capture_plane_floats(B, heads, T, Tk));
    float* maps = tmp.alloc<float>((size_t)B * T * Tk);
    if (!planes || !maps) return FGDM_ERR_NOMEM;
    return time_launches(3, iters, avg_ms, [&]() {
        int rc = attention_capture_launch(dq, C, dk, C, dv, Tkp, o, C, B, heads, T, Tk, d, 0, planes, nullptr);
        if (rc == FGDM_OK && capture == 2) rc = attention_maps_reduce(planes, maps, heads, T, Tk, 0, B, nullptr, Tk, 0, nullptr);
        return rc;
    });
}
int fgdm_bench_attention(int B, int heads, int T, int Tk, int d, int iters, float* avg_ms) {
    return bench_attention(B, heads, T, Tk, d, 0, iters, avg_ms);
}
int fgdm_bench_attention_maps(int B, int heads, int T, int Tk, int d, int with_reduce, int iters, float* avg_ms) {
    return bench_attention(B, heads, T, Tk, d, with_reduce ? 2 : 1, iters, avg_ms);
}

// Micro-benchmark of one GroupNorm / LayerNorm shape on random data: average device ms over `iters` launches.
// kind 0: GroupNorm32(+SiLU) over [B, HW, C0 (+ C1 virtual concat)]; kind 1: LayerNorm over [B * HW, C0].
int fgdm_bench_norm(int kind, int B, int HW, int C0, int C1, int silu, int iters, float* avg_ms) {
    if (!avg_ms || iters <= 0 || B <= 0 || HW <= 0) return FGDM_ERR_ARG;
    const int C = C0 + C1;
    const size_t n0 = (size_t)B * HW * C0, n1 = (size_t)B * HW * (size_t)std::max(C1, 1), n = (size_t)B * HW * C;
    unsigned st = 777u;
    auto rnd = [&]() { st = st * 1664525u + 1013904223u; return ((st >> 9) & 0xffff) / 32768.0f - 1.0f; };
    std::vector<half_t> h0(n0), h1(n1);
    for (auto& v : h0) v = (half_t)rnd();
    for (auto& v : h1) v = (half_t)rnd();
    std::vector<float> g(C), b(C);
    for (int i = 0; i < C; ++i) { g[i] = 1.f + 0.2f * rnd(); b[i] = 0.1f * rnd(); }
    TmpDev tmp;
    half_t* out = tmp.alloc<half_t>(n);
    float* ws = tmp.alloc<float>(groupnorm_ws_floats(B, HW));
    if (!out || !ws) return FGDM_ERR_NOMEM;
    const half_t* d0 = tmp.up(h0);
    const half_t* d1 = C1 ? tmp.up(h1) : nullptr;
    const float* dg = tmp.up(g);
    const float* db = tmp.up(b);
    if (!d0 || !dg || !db) return FGDM_ERR_NOMEM;
    auto run = [&]() {
        return kind == 0 ? groupnorm_launch(d0, C0, d1, C1, B, HW, dg, db, 1e-5f, silu, out, ws, nullptr)
                         : layernorm_launch(d0, B * HW, C0, dg, db, 1e-5f, out, nullptr);
    };
    return time_launches(3, iters, avg_ms, run);
}

}  // extern "C"
