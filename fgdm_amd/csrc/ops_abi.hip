// Op-level test entries of the C ABI (fgdm_op_*, fgdm_debug_*): single kernels and short launch sequences on caller-owned
// buffers, for the per-kernel parity tests.  No engine: they restate the weight packing and the IgemmArgs on their own, and
// share with engine.hip only the launch sequences of engine_shared.h (im2col_conv, vattn_core, conv3_kmap).
#include "engine_shared.h"
#include "replay_plan.h"

// The host-side packing of every entry below.  w [N][Ks] and bias [N] (or null), fp32 on the host or the device, become what the
// GEMM kernels read: a.Wt [igemm_npad(N)][K] fp16 and a.bias [npad] fp32 on the device (owned by `tmp`; pad rows and columns zero).
// Packed row n is source row n, or -- geglu -- the value and the gate rows interleaved in runs of 32 (the 64-column groups whose
// halves the GEGLU epilogue multiplies); packed column k is source column kmap[k] (no kmap: k itself; -1: a pad column).
// With gamma / beta [K] the LayerNorm of A's rows is folded in (IgemmArgs::ln_stats): the weight is fp16(gamma_k w_nk), a.ln_u its
// row sums and the bias gains sum_k beta_k w_nk.
static int op_pack(IgemmArgs& a, TmpDev& tmp, const float* w, const float* bias, int N, int K, int Ks, bool geglu,
                   const int* kmap = nullptr, const float* gamma = nullptr, const float* beta = nullptr) {
    auto host = [](const float* d, size_t n, std::vector<float>& v) { v.resize(n); return hipMemcpy(v.data(), d, n * sizeof(float), hipMemcpyDefault) == hipSuccess; };
    std::vector<float> wh, bh(N, 0.f), g, bt;
    if (!host(w, (size_t)N * Ks, wh) || (bias && !host(bias, N, bh))) return FGDM_ERR_HIP;
    if (gamma && (!host(gamma, K, g) || !host(beta, K, bt))) return FGDM_ERR_HIP;
    const size_t npad = igemm_npad(N);
    std::vector<half_t> pk(npad * (size_t)K, (half_t)0);
    std::vector<float> bp(npad, 0.f), u(gamma ? npad : 0, 0.f);
    for (int pr = 0; pr < N; ++pr) {
        int sr = pr;
        if (geglu) { const int grp = pr >> 6, within = pr & 63; sr = within < 32 ? grp * 32 + within : N / 2 + grp * 32 + (within - 32); }
        const float* row = &wh[(size_t)sr * Ks];
        double us = 0.0, cs = 0.0;
        for (int k = 0; k < K; ++k) {
            const int ks = kmap ? kmap[k] : k;
            if (ks < 0) continue;
            const half_t wq = (half_t)(gamma ? row[ks] * g[k] : row[ks]);
            pk[(size_t)pr * K + k] = wq;
            if (gamma) { us += (double)(float)wq; cs += (double)bt[k] * (double)row[ks]; }
        }
        bp[pr] = gamma ? (float)((double)bh[sr] + cs) : bh[sr];
        if (gamma) u[pr] = (float)us;
    }
    a.Wt = tmp.up(pk); a.bias = tmp.up(bp);
    if (gamma) a.ln_u = tmp.up(u);
    return a.Wt && a.bias && (!gamma || a.ln_u) ? FGDM_OK : FGDM_ERR_NOMEM;
}

// Engine::gemm for the op-level test entries that share a launch sequence with the engine (im2col_conv, vattn_core): the same
// IgemmArgs the engine would build -- its split-K plan included -- with hipMalloc'ed scratch instead of the arena and no timer.
// The caller has filled the operands and the epilogue; synchronise before `tmp` goes out of scope.
static int op_gemm_rows(IgemmArgs& a, const half_t* A, int B, int Ho, int Wo, int K, int rps, TmpDev& tmp, hipStream_t s) {
    a.A0 = A; a.C0 = K; a.A1 = nullptr; a.C1 = 0;
    a.zero = g_zero_page();
    if (!a.zero) return FGDM_ERR_NOMEM;
    a.B = B; a.H = Ho; a.W = Wo; a.Ho = Ho; a.Wo = Wo;
    a.M = B * Ho * Wo; a.K = K; a.mode = IG_LINEAR; a.rows_per_sample = rps;
    if (plan_splitk(a, tmp) != FGDM_OK) return FGDM_ERR_NOMEM;
    return igemm_launch(a, s);
}

// fgdm_op_conv2d for Cin % 64 != 0: the weight in conv3_kmap's column order, as Engine::pack_conv3 packs it, then im2col_conv as
// Engine::conv3 runs it.  x fp16 NHWC with cin_pad channels.
static int op_conv3_im2col(const half_t* x, int Cin, const float* w, const float* bias, const float* rowvec, const half_t* resid,
                           int B, int H, int W, int Cout, int stride, int act, float scale, void* out, hipStream_t s) {
    int cp = 0;
    const std::vector<int> kmap = conv3_kmap(Cin, &cp);
    const int K = (int)kmap.size(), Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    TmpDev tmp;
    IgemmArgs a{};
    const int prc = op_pack(a, tmp, w, bias, Cout, K, Cin * 9, false, kmap.data());
    if (prc != FGDM_OK) return prc;
    half_t* A = tmp.alloc<half_t>((size_t)B * Ho * Wo * K);
    if (!A) return FGDM_ERR_NOMEM;
    a.rowvec = rowvec; a.rv_stride = Cout;
    a.resid = resid; a.ld_res = Cout;
    a.N = Cout; a.act = act; a.out_kind = OUT_F16; a.out = out; a.ld_out = Cout; a.scale = scale;
    const int rc = im2col_conv(x, A, B, H, W, cp, stride, K, s, []() {},
        [&](half_t* Ap, int Bv, int Hv, int Wv, int Kv, int rps) { return op_gemm_rows(a, Ap, Bv, Hv, Wv, Kv, rps, tmp, s); });
    (void)hipStreamSynchronize(s);   // temporaries are freed on return
    return rc;
}

extern "C" {

// ------------------------------------------------------------------------------------ op-level test entries
int fgdm_op_conv2d(const void* x0, int C0, const void* x1, int C1, const float* w, const float* bias, const float* rowvec,
                   const void* resid, int B, int H, int W, int Cout, int ksize, int stride, int upsample, int act,
                   float scale, void* out, void* stream) {
    if (!x0 || !w || !out || (ksize != 1 && ksize != 3)) return FGDM_ERR_ARG;
    if (stride == FGDM_STRIDE2_PAD_BR && (ksize != 3 || upsample)) return FGDM_ERR_ARG;
    hipStream_t s = as_stream(stream);
    const int Cin = C0 + C1, taps = ksize * ksize, K = taps * Cin;
    if (B <= 0 || H <= 0 || W <= 0 || Cout <= 0 || C0 <= 0 || C1 < 0) return FGDM_ERR_ARG;
    if (Cin & 63) {     // the im2col route: exactly the combinations Engine::conv3 accepts on it
        if (ksize != 3 || C1 || x1 || upsample || (stride != 1 && stride != 2)) return FGDM_ERR_ARG;
        return op_conv3_im2col((const half_t*)x0, C0, w, bias, rowvec, (const half_t*)resid, B, H, W, Cout, stride, act, scale, out, s);
    }
    std::vector<int> kmap(K);        // source row [Cin][taps] -> the order the kernels walk K: 64-channel chunk, then tap, then channel
    for (int tap = 0; tap < taps; ++tap)
        for (int c = 0; c < Cin; ++c) kmap[taps == 9 ? ((c >> 6) * 9 + tap) * 64 + (c & 63) : c] = c * taps + tap;
    TmpDev tmp;
    IgemmArgs a{};
    const int prc = op_pack(a, tmp, w, bias, Cout, K, K, false, kmap.data());
    if (prc != FGDM_OK) return prc;
    a.A0 = (const half_t*)x0; a.C0 = C0; a.A1 = (const half_t*)x1; a.C1 = C1;
    a.zero = g_zero_page();
    if (!a.zero) return FGDM_ERR_NOMEM;
    a.rowvec = rowvec; a.rv_stride = Cout;
    a.resid = (const half_t*)resid; a.ld_res = Cout;
    a.B = B; a.H = H; a.W = W;
    a.Ho = H; a.Wo = W; a.mode = IG_LINEAR;
    if (ksize == 3) {
        a.mode = IG_CONV3;
        if (upsample) { a.Ho = 2 * H; a.Wo = 2 * W; a.mode = IG_CONV3_UP2; }
        else if (stride == 2) { a.Ho = (H - 1) / 2 + 1; a.Wo = (W - 1) / 2 + 1; a.mode = IG_CONV3_S2; }
        else if (stride == FGDM_STRIDE2_PAD_BR) {
            if (H < 2 || W < 2) return FGDM_ERR_ARG;
            a.Ho = (H - 2) / 2 + 1; a.Wo = (W - 2) / 2 + 1; a.mode = IG_CONV3_S2_BR;
        }
    }
    a.M = B * a.Ho * a.Wo; a.N = Cout; a.K = K;
    a.act = act; a.out_kind = OUT_F16; a.out = out; a.ld_out = Cout;
    a.rows_per_sample = a.Ho * a.Wo; a.scale = scale;
    if (igemm_up_phase(a)) {        // the engine's dispatch (Engine::gemm): the four summed 2x2 kernels, packed as Engine::pack_conv3 does
        std::vector<float> wh((size_t)Cout * K);
        if (hipMemcpy(wh.data(), w, wh.size() * sizeof(float), hipMemcpyDefault) != hipSuccess) return FGDM_ERR_HIP;
        const half_t* wph = tmp.up(up_phase_pack(wh.data(), Cout, Cin, igemm_npad(Cout)));
        if (!wph) return FGDM_ERR_NOMEM;
        a = igemm_phase_args(a, wph);
    }
    if (plan_splitk(a, tmp) != FGDM_OK) return FGDM_ERR_NOMEM;
    const int rc = igemm_launch(a, s);
    (void)hipStreamSynchronize(s);   // temporaries are freed on return
    return rc;
}

int fgdm_op_linear(const void* x, const float* w, const float* bias, const void* resid, int M, int K, int N, int act,
                   int out_kind, int rows_per_sample, int ld_out, void* out, void* stream) {
    if (!x || !w || !out || (K & 63)) return FGDM_ERR_ARG;
    hipStream_t s = as_stream(stream);
    TmpDev tmp;
    IgemmArgs a{};
    const int prc = op_pack(a, tmp, w, bias, N, K, K, act == ACT_GEGLU);
    if (prc != FGDM_OK) return prc;
    a.A0 = (const half_t*)x; a.C0 = K;
    a.zero = g_zero_page();
    if (!a.zero) return FGDM_ERR_NOMEM;
    const int nout = act == ACT_GEGLU ? N / 2 : N;
    a.resid = (const half_t*)resid; a.ld_res = nout;
    a.B = 1; a.H = 1; a.W = M; a.Ho = 1; a.Wo = M;
    a.M = M; a.N = N; a.K = K; a.mode = IG_LINEAR; a.act = act; a.out_kind = out_kind;
    a.out = out; a.ld_out = ld_out ? ld_out : nout;
    a.rows_per_sample = rows_per_sample ? rows_per_sample : M; a.scale = 1.f;
    const int rc = igemm_launch(a, s);
    (void)hipStreamSynchronize(s);
    return rc;
}

// h = x W1^T + b1 (+ resid), fp16, with the LayerNorm partial sums of its rows produced on the way (from the GEMM's own
// epilogue when the chosen kernel can, else by row_stats), then y = act(LayerNorm(h) W2^T + b2) with the LayerNorm folded
// into the second GEMM: the producer / consumer pair of every transformer-block LayerNorm (attention.py:234-240).
// *slots_used receives the number of partial-sum slots per row (1 = the separate row_stats pass ran).
int fgdm_op_linear_ln_linear(const void* x, const float* w1, const float* b1, const void* resid, const float* gamma,
                             const float* beta, const float* w2, const float* b2, int M, int K1, int C, int N2, int act2,
                             void* h_out, void* y_out, int* slots_used, void* stream) {
    if (!x || !w1 || !gamma || !beta || !w2 || !h_out || !y_out || (K1 & 63) || (C & 63)) return FGDM_ERR_ARG;
    hipStream_t s = as_stream(stream);
    TmpDev tmp;
    IgemmArgs a{}, b{};
    int rc = op_pack(a, tmp, w1, b1, C, K1, K1, false);
    if (rc == FGDM_OK) rc = op_pack(b, tmp, w2, b2, N2, C, C, act2 == ACT_GEGLU, nullptr, gamma, beta);
    if (rc != FGDM_OK) return rc;
    a.A0 = (const half_t*)x; a.C0 = K1; a.zero = g_zero_page();
    a.resid = (const half_t*)resid; a.ld_res = C;
    a.B = 1; a.H = 1; a.W = M; a.Ho = 1; a.Wo = M; a.M = M; a.N = C; a.K = K1; a.mode = IG_LINEAR; a.act = ACT_NONE;
    a.out_kind = OUT_F16; a.out = h_out; a.ld_out = C; a.rows_per_sample = M; a.scale = 1.f;
    if (!a.zero) return FGDM_ERR_NOMEM;
    int slots = igemm_stats_slots(a);
    float* stats = tmp.alloc<float>((size_t)M * std::max(slots, row_stats_slots(C)) * 2);
    if (!stats) return FGDM_ERR_NOMEM;
    if (slots) a.stats_out = stats;
    rc = igemm_launch(a, s);
    if (rc == FGDM_OK && !slots) { slots = row_stats_slots(C); rc = row_stats_launch((const half_t*)h_out, M, C, stats, s); }
    if (slots_used) *slots_used = a.stats_out ? slots : -slots;      // negative: the separate pass produced them
    if (rc != FGDM_OK) { (void)hipStreamSynchronize(s); return rc; }
    b.A0 = (const half_t*)h_out; b.C0 = C; b.zero = a.zero;
    b.ln_stats = stats; b.ln_slots = slots; b.ln_eps = 1e-5f;
    const int nout = act2 == ACT_GEGLU ? N2 / 2 : N2;
    b.B = 1; b.H = 1; b.W = M; b.Ho = 1; b.Wo = M; b.M = M; b.N = N2; b.K = C; b.mode = IG_LINEAR; b.act = act2;
    b.out_kind = OUT_F16; b.out = y_out; b.ld_out = nout; b.rows_per_sample = M; b.scale = 1.f;
    rc = igemm_launch(b, s);
    (void)hipStreamSynchronize(s);
    return rc;
}

// Diagnostic entry of tests/test_gpu_qkv_projection.py; the product path does not call it.
// to_q | to_k | to_v of a self-attention (attention.py:180-186, no bias) as the ONE GEMM Engine::attn_fwd launches: the stacked
// [3C, C] weight over the raw tokens h with norm1 folded in (fold: statistics from row_stats_launch, gamma in the weight, beta W
// in the bias), packed columns [0, 2C) row-major to qk [B T, 2C], [2C, 3C) transposed to vt [B, C, Tp].  vt is not cleared.
int fgdm_op_ln_qkv(const void* h, const float* gamma, const float* beta, const float* wq, const float* wk, const float* wv,
                   int B, int T, int C, int Tp, int fold, void* qk, void* vt, void* stream) {
    if (!h || !wq || !wk || !wv || !qk || !vt) return FGDM_ERR_ARG;
    if (B <= 0 || T <= 0 || C <= 0 || (C % 320) || Tp < T || (Tp & 7)) return FGDM_ERR_ARG;
    if (fold ? (!gamma || !beta) : (gamma || beta)) return FGDM_ERR_ARG;
    if ((long long)B * T > 0x7fffffffLL / (3 * C)) return FGDM_ERR_ARG;
    hipStream_t s = as_stream(stream);
    const int M = B * T, N = 3 * C;
    const size_t cc = (size_t)C * C;
    std::vector<float> w(3 * cc);
    const float* src[3] = {wq, wk, wv};
    for (int i = 0; i < 3; ++i)
        if (hipMemcpy(&w[i * cc], src[i], cc * sizeof(float), hipMemcpyDefault) != hipSuccess) return FGDM_ERR_HIP;
    TmpDev tmp;
    IgemmArgs a{};
    int rc = op_pack(a, tmp, w.data(), nullptr, N, C, C, false, nullptr, fold ? gamma : nullptr, fold ? beta : nullptr);
    if (rc != FGDM_OK) return rc;
    a.A0 = (const half_t*)h; a.C0 = C; a.zero = g_zero_page();
    if (!a.zero) return FGDM_ERR_NOMEM;
    a.B = B; a.H = 1; a.W = T; a.Ho = 1; a.Wo = T; a.M = M; a.N = N; a.K = C; a.mode = IG_LINEAR; a.act = ACT_NONE;
    a.out_kind = OUT_F16; a.out = qk; a.ld_out = 2 * C; a.rows_per_sample = T; a.scale = 1.f;
    a.out2 = vt; a.out_kind2 = OUT_F16_T; a.ld_out2 = Tp; a.split_n = 2 * C;
    if (fold) {
        const int slots = row_stats_slots(C);
        float* stats = tmp.alloc<float>((size_t)M * slots * 2);
        if (!stats) return FGDM_ERR_NOMEM;
        rc = row_stats_launch((const half_t*)h, M, C, stats, s);
        if (rc != FGDM_OK) { (void)hipStreamSynchronize(s); return rc; }
        a.ln_stats = stats; a.ln_slots = slots; a.ln_eps = 1e-5f;
    }
    rc = igemm_launch(a, s);
    (void)hipStreamSynchronize(s);   // temporaries are freed on return
    return rc;
}

int fgdm_debug_force_igemm_cfg(int cfg) { igemm_set_force_cfg(cfg); return FGDM_OK; }

int fgdm_op_groupnorm(const void* x0, int C0, const void* x1, int C1, int B, int HW, const float* gamma, const float* beta,
                      float eps, int silu, void* out, void* stream) {
    if (!x0 || !gamma || !beta || !out) return FGDM_ERR_ARG;
    hipStream_t s = as_stream(stream);
    float* ws = nullptr;
    if (hipMalloc(&ws, groupnorm_ws_floats(B, HW) * sizeof(float)) != hipSuccess) return FGDM_ERR_NOMEM;
    const int rc = groupnorm_launch((const half_t*)x0, C0, (const half_t*)x1, C1, B, HW, gamma, beta, eps, silu, (half_t*)out, ws, s);
    (void)hipStreamSynchronize(s);
    (void)hipFree(ws);
    return rc;
}
int fgdm_op_layernorm(const void* x, int rows, int C, const float* gamma, const float* beta, float eps, void* out, void* stream) {
    if (!x || !gamma || !beta || !out) return FGDM_ERR_ARG;
    return layernorm_launch((const half_t*)x, rows, C, gamma, beta, eps, (half_t*)out, as_stream(stream));
}
int fgdm_op_attention(const void* q, int ldq, const void* k, int ldk, const void* vt, int ldvt, void* o, int ldo, int B,
                      int heads, int T, int Tk, int d, void* stream) {
    if (!q || !k || !vt || !o) return FGDM_ERR_ARG;
    return attention_launch((const half_t*)q, ldq, (const half_t*)k, ldk, (const half_t*)vt, ldvt, (half_t*)o, ldo, B, heads, T, Tk, d, 0, as_stream(stream));
}
// Diagnostic entries of tests/test_gpu_attention_calls.py: the flag the engine's own calls pass, the kernel the dispatch chose,
// and the text encoder's attention kernel on its own.
int fgdm_op_attention_ex(const void* q, int ldq, const void* k, int ldk, const void* vt, int ldvt, void* o, int ldo, int B,
                         int heads, int T, int Tk, int d, int q_prescaled, void* stream) {
    if (!q || !k || !vt || !o) return FGDM_ERR_ARG;
    return attention_launch((const half_t*)q, ldq, (const half_t*)k, ldk, (const half_t*)vt, ldvt, (half_t*)o, ldo, B, heads, T, Tk, d,
                            q_prescaled ? 1 : 0, as_stream(stream));
}
int fgdm_debug_last_attention_kernel(void) { return attention_last_kernel(); }
// Diagnostic entry of tests/test_gpu_attention_maps.py: fgdm_op_attention_ex through the capturing instantiations, plus the head
// reduction, as the engine's capture runs them; the per-head planes are scratch of this call (synchronises before it frees them).
int fgdm_op_cross_attention_maps(const void* q, int ldq, const void* k, int ldk, const void* vt, int ldvt, void* o, int ldo, float* maps,
                                 int B, int heads, int T, int Tk, int d, int q_prescaled, void* stream) {
    if (!q || !k || !vt || !o || !maps) return FGDM_ERR_ARG;
    if (B <= 0 || heads <= 0 || T <= 0 || Tk <= 0 || Tk > FGDM_ATTENTION_CAPTURE_MAX_KEYS) return FGDM_ERR_ARG;
    if (d != 40 && d != 64 && d != 80 && d != 160) return FGDM_ERR_ARG;
    hipStream_t s = as_stream(stream);
    TmpDev tmp;
    float* planes = tmp.alloc<float>(attention_capture_plane_floats(B, heads, T, Tk));
    if (!planes) return FGDM_ERR_NOMEM;
    int rc = attention_capture_launch((const half_t*)q, ldq, (const half_t*)k, ldk, (const half_t*)vt, ldvt, (half_t*)o, ldo, B, heads, T, Tk,
                                      d, q_prescaled ? 1 : 0, planes, s);
    if (rc == FGDM_OK) rc = attention_maps_reduce(planes, maps, heads, T, Tk, 0, B, nullptr, Tk, 0, s);
    if (hipStreamSynchronize(s) != hipSuccess && rc == FGDM_OK) rc = FGDM_ERR_HIP;
    return rc;
}
int fgdm_op_small_attention(const void* qkv, int ld, int koff, int voff, void* out, int ldo, int B, int heads, int T, int d,
                            int causal, void* stream) {
    if (!qkv || !out) return FGDM_ERR_ARG;
    return small_attention_launch((const half_t*)qkv, ld, koff, voff, (half_t*)out, ldo, B, heads, T, d, causal, as_stream(stream));
}

// Diagnostic entries of tests/test_gpu_narrow_ops.py; the product path does not call them.
// The per-image loop of Engine::vattn_fwd (vattn_core) on caller-owned q / k / vt / out, with S and P of its own.
int fgdm_op_vae_attention(const void* q, const void* k, const void* vt, void* out, int B, int T, int C, void* stream) {
    if (!q || !k || !vt || !out || B <= 0 || T <= 0 || C <= 0 || (T & 63) || (C & 63)) return FGDM_ERR_ARG;
    hipStream_t s = as_stream(stream);
    TmpDev tmp;
    float* S = tmp.alloc<float>((size_t)T * T);
    half_t* P = tmp.alloc<half_t>((size_t)T * T);
    if (!S || !P) return FGDM_ERR_NOMEM;
    bool softmax_failed = false;
    const int rc = vattn_core((const half_t*)q, (const half_t*)k, (const half_t*)vt, (half_t*)out, S, P, B, T, C, s, &softmax_failed,
        [&](const half_t* Wt, int N, int K, const half_t* A, int M, int out_kind, void* o, int ld_out, float scale) {
            IgemmArgs a{};
            a.Wt = Wt; a.N = N; a.act = ACT_NONE; a.out_kind = out_kind; a.out = o; a.ld_out = ld_out; a.scale = scale;
            return op_gemm_rows(a, A, 1, 1, M, K, M, tmp, s);
        });
    (void)hipStreamSynchronize(s);   // S and P are freed on return
    return rc;
}
// Pass-throughs to the host launchers of elementwise.hip, pointer / shape checks in front.
int fgdm_op_softmax_rows(const float* S, void* P, int rows, int cols, void* stream) {
    if (!S || !P || rows <= 0 || cols <= 0) return FGDM_ERR_ARG;
    return softmax_rows(S, (half_t*)P, rows, cols, as_stream(stream));
}
int fgdm_op_nchw_to_nhwc(const float* x, void* y, int B, int C, int HW, int Cpad, void* stream) {
    if (!x || !y || B <= 0 || C <= 0 || HW <= 0 || Cpad < C) return FGDM_ERR_ARG;
    return nchw_f32_to_nhwc_f16(x, (half_t*)y, B, C, HW, Cpad, as_stream(stream));
}
// Diagnostic entry of tests/test_gpu_hybrid.py: the engine's first-layer pack for in_channels > 4 on caller-owned buffers.
int fgdm_op_pack_xcat(const float* x, const void* cc16, int B, int Bc, int Cc, int H, int W, int cin_pad, void* out, void* stream) {
    if (!x || !cc16 || !out || H <= 0 || W <= 0) return FGDM_ERR_ARG;
    return pack_xcat(x, (const half_t*)cc16, (half_t*)out, B, Bc, Cc, H * W, cin_pad, as_stream(stream));
}
int fgdm_op_nhwc_to_nchw(const void* x, float* y, int B, int C, int HW, void* stream) {
    if (!x || !y || B <= 0 || C <= 0 || HW <= 0) return FGDM_ERR_ARG;
    return nhwc_f16_to_nchw_f32((const half_t*)x, y, B, C, HW, as_stream(stream));
}
int fgdm_op_avgpool2(const void* x, void* y, int B, int H, int W, int C, void* stream) {
    if (!x || !y || B <= 0 || H <= 0 || W <= 0 || C <= 0 || (C & 7) || (H & 1) || (W & 1)) return FGDM_ERR_ARG;
    return avgpool2((const half_t*)x, (half_t*)y, B, H, W, C, as_stream(stream));
}
int fgdm_op_transpose_pad(const void* v, void* vt, int B, int Tk, int C, int Tkpad, void* stream) {
    if (!v || !vt || B <= 0 || Tk <= 0 || C <= 0 || Tkpad < Tk) return FGDM_ERR_ARG;
    return transpose_pad_keys((const half_t*)v, (half_t*)vt, B, Tk, C, Tkpad, as_stream(stream));
}
int fgdm_op_timestep_embed(const int64_t* t, const float* t_float, void* y, int B, int dim, int rows_pad, void* stream) {
    if ((!t && !t_float) || !y || B <= 0 || dim < 2 || (dim & 1) || rows_pad < B) return FGDM_ERR_ARG;
    return timestep_embed(t, t_float, (half_t*)y, B, dim, rows_pad, as_stream(stream));
}
int fgdm_op_add_f16(const void* a, const void* b, void* y, int64_t n, void* stream) {
    if (!a || !b || !y || n <= 0 || (n & 7)) return FGDM_ERR_ARG;
    return add_f16((const half_t*)a, (const half_t*)b, (half_t*)y, (size_t)n, as_stream(stream));
}

// Diagnostic entries of tests/test_gpu_fp32_ops.py; the product path does not call them.
// Pass-throughs to the fp32-side launchers of the text encoder (text.hip, norm.hip, elementwise.hip) and of the first stage
// (elementwise.hip), pointer / shape checks in front.
int fgdm_op_embed_tokens(const int64_t* ids, const float* tok, const float* pos, float* out, int rows, int T, int W, int vocab,
                         void* stream) {
    if (!ids || !tok || !pos || !out || rows <= 0 || T <= 0 || W <= 0 || (W & 7) || vocab <= 0) return FGDM_ERR_ARG;
    return embed_tokens(ids, tok, pos, out, rows, T, W, vocab, as_stream(stream));
}
int fgdm_op_layernorm32(const float* x, int rows, int C, const float* gamma, const float* beta, float eps, void* out16, float* out32,
                        void* stream) {
    if (!x || !gamma || !beta || rows <= 0 || C <= 0 || (C & 3) || (!out16 == !out32)) return FGDM_ERR_ARG;
    return layernorm32_launch(x, rows, C, gamma, beta, eps, (half_t*)out16, out32, as_stream(stream));
}
int fgdm_op_add_f16_to_f32(const float* a, const void* b16, float* y, int64_t n, void* stream) {
    if (!a || !b16 || !y || n <= 0) return FGDM_ERR_ARG;
    return add_f16_to_f32(a, (const half_t*)b16, y, (size_t)n, as_stream(stream));
}
int fgdm_op_f32_to_f16(const float* x, void* y, int64_t n, void* stream) {
    if (!x || !y || n <= 0) return FGDM_ERR_ARG;
    return f32_to_f16(x, (half_t*)y, (size_t)n, as_stream(stream));
}
int fgdm_op_silu_f32_to_f16(const float* x, void* y, int64_t n, void* stream) {
    if (!x || !y || n <= 0) return FGDM_ERR_ARG;
    return silu_f32_to_f16(x, (half_t*)y, (size_t)n, as_stream(stream));
}
int fgdm_op_vae_prequant(const float* z, const float* wb, float scale, void* y, int B, int HW, void* stream) {
    if (!z || !wb || !y || B <= 0 || HW <= 0) return FGDM_ERR_ARG;
    return vae_prequant(z, wb, scale, (half_t*)y, B, HW, as_stream(stream));
}
int fgdm_op_vae_moments(const float* h, const float* wb, float* moments, int B, int HW, void* stream) {
    if (!h || !wb || !moments || B <= 0 || HW <= 0) return FGDM_ERR_ARG;
    return vae_moments(h, wb, moments, B, HW, as_stream(stream));
}

// Diagnostic entry of tests/test_gpu_ddim_loop.py: one launch of the device DDIM loop's step kernel on caller-owned buffers.
int fgdm_op_ddim_loop_step(const float* x, const float* e_cond, const float* e_uncond, float cfg_scale, float a_t, float a_prev,
                           float sigma_t, float sqrt_one_minus_at, const float* noise, const float* mask, const float* x0,
                           const float* q_noise, float sqrt_ac_next, float sqrt_one_minus_ac_next, float* x_out, float* xin_a,
                           float* xin_b, float* log_x, float* log_pred_x0, int64_t n, void* stream) {
    if (!x || n <= 0 || (e_uncond && !e_cond) || (mask && (!x0 || !q_noise))) return FGDM_ERR_ARG;
    LoopStep a{};
    a.io = StepIO{x, e_cond, e_uncond, x_out, xin_a, xin_b, log_x, cfg_scale, (size_t)n};
    a.noise = noise; a.mask = mask; a.x0 = x0; a.qnoise = q_noise; a.log_p0 = log_pred_x0;
    a.a_t = a_t; a.a_prev = a_prev; a.sigma = sigma_t; a.s1m = sqrt_one_minus_at;
    a.sa_next = sqrt_ac_next; a.s1m_next = sqrt_one_minus_ac_next; a.mode = LOOP_PLAIN;
    return loop_step(a, as_stream(stream));
}

// Diagnostic entries of tests/test_gpu_multistep_loop.py: one launch of the device PLMS / DPM-Solver++ loop's step kernel on
// caller-owned buffers.
int fgdm_op_plms_loop_step(const float* x, const float* e_cond, const float* e_uncond, float cfg_scale, int mode, int order,
                           const float* e1, const float* e2, const float* e3, float* e_out, float a_t, float a_prev,
                           float sqrt_one_minus_at, const float* mask, const float* x0, const float* q_noise, float sqrt_ac_next,
                           float sqrt_one_minus_ac_next, float* x_out, float* xin_a, float* xin_b, float* log_x, float* log_pred_x0,
                           int64_t n, void* stream) {
    if (n <= 0 || (e_cond && mode == LOOP_PLAIN)) return FGDM_ERR_ARG;      // the plain (DDIM) mode is no mode of this entry
    LoopStep a{};
    a.io = StepIO{x, e_cond, e_uncond, x_out, xin_a, xin_b, log_x, cfg_scale, (size_t)n};
    a.e1 = e1; a.e2 = e2; a.e3 = e3; a.mask = mask; a.x0 = x0; a.qnoise = q_noise; a.e_out = e_out; a.log_p0 = log_pred_x0;
    a.a_t = a_t; a.a_prev = a_prev; a.s1m = sqrt_one_minus_at; a.sa_next = sqrt_ac_next;
    a.s1m_next = sqrt_one_minus_ac_next; a.mode = mode; a.order = order;
    return loop_step(a, as_stream(stream));
}

int fgdm_op_dpmpp_loop_step(const float* x, const float* e_cond, const float* e_uncond, float cfg_scale, float inv_alpha,
                            float neg_sigma_over_alpha, const float* m1, int update_kind, float c1, float cm0, float cm1,
                            float* m0_out, float* x_out, float* xin_a, float* xin_b, int64_t n, void* stream) {
    if (n <= 0) return FGDM_ERR_ARG;
    DpmppLoopStep a{};
    a.io = StepIO{x, e_cond, e_uncond, x_out, xin_a, xin_b, nullptr, cfg_scale, (size_t)n};
    a.m1 = m1; a.m0_out = m0_out; a.inv_alpha = inv_alpha; a.neg_sigma_over_alpha = neg_sigma_over_alpha; a.c1 = c1; a.cm0 = cm0; a.cm1 = cm1;
    a.kind = update_kind;
    return dpmpp_loop_step(a, as_stream(stream));
}

// One launch of the DPM-Solver program loop's step kernel on caller-owned buffers: the per-step route of fgdm_amd/dpm_solver.py and
// tests/test_gpu_dpm_solver_loop.py.
int fgdm_op_dpm_program_step(const float* x_eval, const float* e_cond, const float* e_uncond, float cfg_scale, float conv_x, float conv_e,
                             float* base, float* hist0, float* hist1, float* hist2, int slot, int nterms, const int32_t* planes,
                             const float* coefs, float* x_out, float* xin_a, float* xin_b, int64_t n, void* stream) {
    if (n <= 0) return FGDM_ERR_ARG;
    DpmProgramStep a{};
    float* const pl[4] = {base, hist0, hist1, hist2};
    if (dpm_program_terms(a, pl, slot, nterms, planes, coefs) != FGDM_OK) return FGDM_ERR_ARG;
    a.io = StepIO{x_eval, e_cond, e_uncond, x_out, xin_a, xin_b, nullptr, cfg_scale, (size_t)n};
    a.conv_x = conv_x; a.conv_e = conv_e;
    return dpm_program_step(a, as_stream(stream));
}

// Diagnostic entries of tests/test_gpu_ancestral_loop.py: one launch of the device ancestral loop's / the device DDIM inversion's
// step kernel on caller-owned buffers.
int fgdm_op_ancestral_loop_step(const float* x, const float* eps, float sqrt_recip_ac, float sqrt_recipm1_ac, float coef1, float coef2,
                                float std, const float* noise, const float* mask, const float* x0, const float* q_noise,
                                float sqrt_ac_t, float sqrt_one_minus_ac_t, float* x_out, float* xin, float* log_x, int64_t n,
                                void* stream) {
    if (n <= 0) return FGDM_ERR_ARG;
    AncestralLoopStep a{};
    a.io = StepIO{x, eps, nullptr, x_out, xin, nullptr, log_x, 0.f, (size_t)n};
    a.noise = noise; a.mask = mask; a.x0 = x0; a.qnoise = q_noise;
    a.cr = sqrt_recip_ac; a.crm1 = sqrt_recipm1_ac; a.c1 = coef1; a.c2 = coef2; a.std = std;
    a.sa_t = sqrt_ac_t; a.s1m_t = sqrt_one_minus_ac_t;
    return ancestral_loop_step(a, as_stream(stream));
}

int fgdm_op_invert_loop_step(const float* x, const float* e_cond, const float* e_uncond, float cfg_scale, float cx, float ce,
                             float* x_out, float* xin_a, float* xin_b, float* log_x, int64_t n, void* stream) {
    if (n <= 0) return FGDM_ERR_ARG;
    InvertLoopStep a{};
    a.io = StepIO{x, e_cond, e_uncond, x_out, xin_a, xin_b, log_x, cfg_scale, (size_t)n};
    a.cx = cx; a.ce = ce;
    return invert_loop_step(a, as_stream(stream));
}

// Diagnostic entry of tests/test_gpu_device_noise.py: the raw words of the loops' generator (noise.h).
int fgdm_op_rand_bits(uint64_t seed, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t* out, int64_t n_blocks, void* stream) {
    if (n_blocks <= 0) return FGDM_ERR_ARG;
    const uint32_t c[4] = {c0, c1, c2, c3};
    return rand_bits(seed, c, out, (size_t)n_blocks, as_stream(stream));
}

// The LoRA merge kernel on caller-owned device buffers (tests/test_gpu_lora.py; fgdm_amd/lora.py merges each touched tensor with it)
int fgdm_op_lora_merge(const float* W, const float* up, const float* down, float s, int O, int I, int r, float* out, void* stream) {
    if (!W || !up || !down || !out || O <= 0 || I <= 0 || r < 1 || r > 128 || O > 65535 * 16) return FGDM_ERR_ARG;
    return lora_merge(W, up, down, s, O, I, r, out, as_stream(stream));
}

// Host-only entry of tests/test_replay_plan.py: the planner of replay_plan.h on caller-made walks.  Never touches the device.
int fgdm_replay_plan(int n_walks, const int32_t* lens, const uint64_t* key, const uint32_t* grid_x, const uint64_t* shape, int group_max,
                     int chunk, int32_t* out, int out_cap, int* limits) {
    if (limits) { limits[0] = REPLAY_LOOK; limits[1] = FGDM_MAX_GROUP; }
    if (n_walks < 0 || group_max < 1 || out_cap < 0 || (n_walks && !lens) || (out_cap && !out)) return FGDM_ERR_ARG;
    std::vector<PlanWalk> walks(n_walks);
    size_t u = 0;
    for (int w = 0; w < n_walks; ++w) {
        if (lens[w] < 0 || (lens[w] && (!key || !grid_x || !shape))) return FGDM_ERR_ARG;
        for (int i = 0; i < lens[w]; ++i, ++u) walks[w].push_back(PlanUnit{key[u], grid_x[u], shape[u]});
    }
    std::vector<int32_t> steps;
    replay_plan_chunked(walks.data(), n_walks, chunk, group_max, REPLAY_LOOK, steps);
    for (size_t i = 0; i < steps.size() && i < (size_t)out_cap; ++i) out[i] = steps[i];
    return (int)steps.size();
}

}  // extern "C"
