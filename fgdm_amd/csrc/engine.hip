// FG-DM sampling engine: weight repacking of the model graph (model.h: SD-v1.x UNet + FG-DM adapter + ControlNet twin encoders,
// first stage, text encoder) into kernel layouts, activation workspace, and the forward passes, all as launches of the
// hand-written gfx950 kernels in this directory.  No torch, no BLAS: only the HIP runtime.
//
// Reference structure being reproduced (file:line in the reference checkout):
//   UNetModel.forward               ldm/modules/diffusionmodules/openaimodel.py:808-884 (753-806 original)
//   ResBlock._forward               openaimodel.py:275-301
//   SpatialTransformer & friends    ldm/modules/attention.py:152-292
//   Adapter                         ldm/modules/encoders/adapter.py:280-346
//   ControlNet / ControlledUnet     controlnet/cldm/cldm.py:27-50, 545-813, 836-849
#include "model.h"
#include "arena.h"
#include "knobs.h"
#include "replay.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

namespace {

// Built-in kernel timer: when enabled, every launch is bracketed by HIP events recorded on the launch stream
// (the same stream the kernels run on), so per-kernel-class device time, launch counts and the ALGORITHMIC
// flops / bytes of exactly those launches can be read back without an external profiler.
enum ProfClass { PC_IGEMM = 0, PC_ATTN = 1, PC_NORM = 2, PC_ELEM = 3, PC_COUNT = 4 };
struct Prof final : LaunchTimer {
    bool on = false;
    std::vector<hipEvent_t> pool;
    size_t used = 0;
    struct Rec { int cls; size_t e0, e1; double w; char tag[56]; };
    std::vector<Rec> recs;
    double work[PC_COUNT] = {0, 0, 0, 0};     // flops (igemm, attention) or bytes (norm, elementwise)
    double bytes[PC_COUNT] = {0, 0, 0, 0};    // algorithmic HBM bytes (each operand once)
    hipEvent_t get() {
        if (used == pool.size()) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) return nullptr; pool.push_back(e); }
        return pool[used++];
    }
    // Only every `stride`-th launch is bracketed: two event packets per launch cost ~3 % of a 41k-launch sampling
    // step; a stride coprime with the number of bracketed launches per evaluation (it varies with the ControlNet count and the
    // grouping knobs) samples every shape uniformly.
    int stride = 1;
    long counter = 0;
    bool armed = false;
    // bytes: algorithmic HBM bytes of the bracketed launch (counted only when the bracket is taken)
    void begin(int cls, hipStream_t s, double w, const char* tag = "", double nbytes = 0.0) override {
        if (fgdm_recording()) {                       // recording: the bracket becomes two ops around the launch it encloses
            if (on) fgdm_record_bracket_begin(cls, w, nbytes, tag);
            return;
        }
        armed = false;
        if (!on || (counter++ % stride) != 0) return;
        armed = true;
        hipEvent_t e = get();
        if (!e) return;
        (void)hipEventRecord(e, s);
        Rec r{cls, used - 1, 0, w, {0}};
        snprintf(r.tag, sizeof(r.tag), "%s", tag);
        recs.push_back(r);
        work[cls] += w;
        bytes[cls] += nbytes;
    }
    void end(hipStream_t s) override {
        if (fgdm_recording()) {
            if (on) fgdm_record_bracket_end();
            return;
        }
        if (!on || !armed || recs.empty()) return;
        armed = false;
        hipEvent_t e = get();
        if (!e) return;
        (void)hipEventRecord(e, s);
        recs.back().e1 = used - 1;
    }
};

}  // namespace

struct fgdm_engine : Model {
    int device = -1;
    bool device_ready = false, finalized = false;
    // cross-attention K / V^T of a registered context (fgdm_set_context): constant over the denoising steps
    struct CtxKV { Tensor k, vt; };
    std::unordered_map<const Layer*, CtxKV> ctx_cache;
    int ctx_B = 0, ctx_T = 0;
    int ctx_tokens = 77;                 // tokens behind every ctx / cond / uncond pointer (fgdm_set_context_tokens); 77 = one CLIP chunk
    // Cross-attention maps (fgdm_attention_capture_*): the plan, one accumulator [rows, T, n_tok] per selected UNet block and the
    // per-head planes the capturing kernels write (one scratch buffer: the launches that use it are ordered on the stream).  The
    // ControlNets' layers are not in `planes`, so their cross-attentions are never captured.  capturing: inside an apply_model only.
    struct CapPlane { int block = 0, heads = 0, h = 0, w = 0; float* acc = nullptr; };
    struct Capture {
        bool on = false, capturing = false;
        int rows_sel = 0, mode = 0, Tk = 0;
        int B = 0, H = 0, W = 0;         // the evaluations' batch and latent size (0: not fixed yet, nothing allocated)
        int row0 = 0, rows = 0, n_evals = 0;
        std::vector<int> tokens;
        int* tok_dev = nullptr;
        float* head_planes = nullptr;
        std::vector<const Layer*> order;                       // the UNet's transformer blocks in walk order
        std::unordered_map<const Layer*, CapPlane> planes;     // the selected ones
    } cap;
    // Device noise (fgdm_loop_noise_set): while `on`, a loop call makes the noise it is not handed inside its step kernels (noise.h)
    struct LoopNoise {
        bool on = false;
        uint64_t seed = 0;
        int32_t first_sample = 0, first_step = 0, repeat = 0;
        float temperature = 1.f;
    } loop_noise;
    // the generator of a launch at local walk position `i`: stream 0 there, stream 1 at local position `qi`
    NoiseGen noise_gen(int H, int W, int i, int qi, bool step_on, bool q_on) const {
        NoiseGen g{};
        if (!loop_noise.on || (!step_on && !q_on)) return g;
        g.key0 = (uint32_t)loop_noise.seed; g.key1 = (uint32_t)(loop_noise.seed >> 32);
        g.first_sample = (uint32_t)loop_noise.first_sample; g.per_sample = 4u * (uint32_t)H * (uint32_t)W;
        g.step = (uint32_t)loop_noise.first_step + (uint32_t)i; g.q_step = (uint32_t)loop_noise.first_step + (uint32_t)qi;
        g.temperature = loop_noise.temperature; g.repeat = loop_noise.repeat;
        g.step_on = step_on; g.q_on = q_on;
        return g;
    }
    void capture_free() {
        for (auto& kv : cap.planes) { (void)hipFree(kv.second.acc); kv.second.acc = nullptr; }
        (void)hipFree(cap.tok_dev); (void)hipFree(cap.head_planes);
        cap.tok_dev = nullptr; cap.head_planes = nullptr;
        cap.B = cap.H = cap.W = 0;
    }
    void capture_off() { capture_free(); cap = Capture{}; }
    size_t capture_plane_floats(const CapPlane& p) const { return (size_t)cap.rows * p.h * p.w * cap.tokens.size(); }
    // the accumulators for evaluations of B rows on an H x W latent: every selected block's h x w follows from its place in the walk
    int capture_alloc(int B, int H, int W) {
        capture_free();
        const bool half = cap.rows_sel != FGDM_CAPTURE_ROWS_ALL;
        if (half && (B & 1)) return fail(FGDM_ERR_STATE, "attention capture: the conditional / unconditional half of an odd batch");
        cap.rows = half ? B / 2 : B;
        cap.row0 = cap.rows_sel == FGDM_CAPTURE_ROWS_COND ? B / 2 : 0;      // cat([uncond, cond])
        int h = H, w = W;
        size_t scratch = 0;
        auto walk = [&](const Block& blk) -> int {
            for (const Layer& l : blk) {
                if (l.type == L_DOWN) { h = (h + 1) / 2; w = (w + 1) / 2; }
                if (l.type == L_UP) { h *= 2; w *= 2; }
                auto it = l.type == L_ATTN ? cap.planes.find(&l) : cap.planes.end();
                if (it == cap.planes.end()) continue;
                CapPlane& p = it->second;
                p.h = h; p.w = w; p.heads = l.heads;
                scratch = std::max(scratch, attention_capture_plane_floats(B, l.heads, h * w, cap.Tk));
            }
            return FGDM_OK;
        };
        CHK0(for_each_block(unet, false, walk));
        bool ok = hipMalloc(&cap.tok_dev, cap.tokens.size() * sizeof(int)) == hipSuccess &&
                  hipMemcpy(cap.tok_dev, cap.tokens.data(), cap.tokens.size() * sizeof(int), hipMemcpyHostToDevice) == hipSuccess &&
                  hipMalloc(&cap.head_planes, scratch * sizeof(float)) == hipSuccess;
        for (auto& kv : cap.planes) {
            const size_t bytes = capture_plane_floats(kv.second) * sizeof(float);
            ok = ok && hipMalloc(&kv.second.acc, bytes) == hipSuccess && hipMemset(kv.second.acc, 0, bytes) == hipSuccess;
        }
        if (!ok) { capture_free(); return fail(FGDM_ERR_NOMEM, "hipMalloc (attention capture)"); }
        cap.B = B; cap.H = H; cap.W = W;
        cap.n_evals = 0;
        return FGDM_OK;
    }
    // apply_model, before its first launch: is this an evaluation the plan captures?
    int capture_begin(int B, int H, int W) {
        if (cap.Tk != ctx_tokens) return fail(FGDM_ERR_STATE, "attention capture: the context token count changed after the plan was set");
        if (!cap.B) CHK0(capture_alloc(B, H, W));
        if (B != cap.B || H != cap.H || W != cap.W)
            return fail(FGDM_ERR_STATE, "attention capture: this evaluation's batch or latent size is not the one the accumulators were made for");
        cap.capturing = true;
        ++cap.n_evals;
        return FGDM_OK;
    }
    // c_concat of a UNet fed cat([x] + c_concat, 1) (in_channels > 4; fgdm_set_concat): loop-invariant, kept as fp16 NHWC
    // [Bc, H W, in_channels - 4] (persistent hipMalloc, like a ControlNet's cached hint)
    Tensor ccat;
    Arena arena;
    half_t* zero = nullptr;
    int cur_comp = -1;            // the component being packed: its Component::allocs takes the uploads
    // Weight updates of a finalized engine (fgdm_weights_*): the tensors supplied since begin_update, staged on the host until the
    // commit re-packs the units that own them IN PLACE; the size of every packed buffer; the snapshot (device copies of units'
    // buffers, put back by fgdm_weights_restore)
    bool upd_open = false, in_place = false;
    std::unordered_map<std::string, std::vector<float>> upd;
    std::unordered_map<void*, size_t> alloc_bytes;
    struct Snap { void* dst; void* copy; size_t bytes; };
    std::vector<Snap> snap;
    // LayerNorms of the transformer blocks folded into the GEMMs they feed (default) or run as kernels of their own
    // (FGDM_LN_FOLD=0 at fgdm_create: the A/B switch for tools/ab_bench.sh; numerics differ only in rounding points)
    bool ln_fold = true;
    hipStream_t s = nullptr;      // stream of the call in flight
    // FGDM_TWIN_STREAMS=1: the ControlNets run on a second stream (own arena: an arena's block reuse relies on stream order) next
    // to the UNet encoder + middle block, which they do not depend on (cldm.py:40,46: the UNet takes `control` only after its middle
    // block); their zero-convs are applied on the main stream behind a join event
    // the ControlNets' workspaces: ONE ARENA PER ControlNet (round 4).  A recorded walk hands blocks out and takes them back at
    // RECORD time, so two walks recorded from one arena share blocks; replayed INTERLEAVED (grouped launches) they would overwrite
    // each other (three ControlNets at full size gave non-finite latents in round 3, fixed then by a hand-derived two-arena rule).
    // With an arena of its own every walk may be replayed next to any other.  cn_arena[0] also serves the second stream.
    // OWNERSHIP (arena.h): every block is held by one Act / Buf / LnStats handle, which gives it back to the arena it came from --
    // not to `ar`, which RecordScope moves -- when it is destroyed, reset() or assigned over.  A function that consumes its input
    // takes the handle by value, one that only reads takes const Tensor&; an early `return fail(...)` unwinds what the call holds.
    // The one thing unwinding cannot order by itself is the second stream: see SecondStreamGuard in apply_model_walk.
    std::vector<std::unique_ptr<Arena>> cn_arena;
    Arena* ar = &arena;           // arena of the stream being enqueued: where talloc / balloc take NEW blocks from
    hipStream_t s2 = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    bool twin_streams = false;
    // FGDM_PAIR_LAUNCH (default on): the UNet encoder + middle block and the ControlNets are RECORDED (common.h, "deferred
    // launches") and replayed in lockstep on the one stream, twin launches fused into grouped launches (replay.h: fgdm_replay)
    bool pair_launch = true;
    int group_max = FGDM_MAX_GROUP;      // FGDM_GROUP_MAX (read at fgdm_create): 2 = round 3's pairwise replay; the A/B knob
    bool gn_group = true;                // FGDM_GN_GROUP (read at fgdm_create): the twins' single-pass GroupNorm launches group too
    ReplayStats replay_stats;            // behind fgdm_launch_stats
    using Act = Owned<Tensor>;           // an fp16 activation of the workspace and the arena that served it
    static Act borrow(const Tensor& t) { return Act(t, nullptr); }      // a view in a handle's clothes: owns nothing
    struct Deferred { const GemmW* w; Act src; int idx; float scale; };  // a zero-conv the caller applies later; holds its input
    Prof prof;

    // ------------------------------------------------------------------------------------ weight packing
    const ParamSlot* slot(const std::string& name) {
        auto it = params.find(name);
        if (it == params.end() || !it->second.loaded) { err = "parameter not loaded: " + name; return nullptr; }
        return &it->second;
    }
    // `into`: the buffer the unit holds now.  A weight update (fgdm_weights_commit_update) writes the new bytes over it -- same
    // shapes, so the same size -- and every pointer the engine handed out stays good; a first packing allocates.
    template <typename T> T* upload(const std::vector<T>& h, T* into = nullptr) {
        if (in_place) {
            auto it = into ? alloc_bytes.find(into) : alloc_bytes.end();
            if (it == alloc_bytes.end() || it->second < h.size() * sizeof(T)) return nullptr;
            return hipMemcpy(into, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess ? into : nullptr;
        }
        T* d = nullptr;
        const size_t bytes = std::max<size_t>(h.size() * sizeof(T), 256);
        if (hipMalloc(&d, bytes) != hipSuccess) return nullptr;
        if (hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
        comps[cur_comp].allocs.push_back(d);
        alloc_bytes[d] = bytes;
        return d;
    }
    // rows: list of (source float*, n_rows) stacked along N; each source is [n][K_src] row-major;
    // kmap(k_packed) -> k_src or -1.  row_perm maps packed row -> stacked source row (GEGLU interleave).
    int pack_rows(GemmW& g, const std::vector<std::pair<const float*, int>>& srcs, int K_src, int K,
                  const std::vector<int>& kmap, const std::vector<const float*>& biases, bool geglu,
                  const std::vector<float>& src_scale = {}, const float* ln_gamma = nullptr, const float* ln_beta = nullptr) {
        int N = 0;
        for (auto& s : srcs) N += s.second;
        const size_t npad = igemm_npad(N);
        std::vector<half_t> w(npad * (size_t)K, (half_t)0);
        std::vector<float> bias(npad, 0.f), lnu(ln_gamma ? npad : 0, 0.f);
        std::vector<const float*> rowp(N);
        std::vector<float> bflat(N, 0.f), rscale(N, 1.f);
        int r = 0;
        for (size_t si = 0; si < srcs.size(); ++si)
            for (int i = 0; i < srcs[si].second; ++i, ++r) {
                rowp[r] = srcs[si].first + (size_t)i * K_src;
                if (si < biases.size() && biases[si]) bflat[r] = biases[si][i];
                if (si < src_scale.size()) rscale[r] = src_scale[si];      // multiplied in fp32 BEFORE the fp16 rounding
            }
        for (int pr = 0; pr < N; ++pr) {
            int sr = pr;
            if (geglu) {   // packed 64-row groups = [32 value rows | 32 gate rows]; gate rows live at N/2 + i
                const int grp = pr >> 6, within = pr & 63;
                sr = within < 32 ? grp * 32 + within : N / 2 + grp * 32 + (within - 32);
            }
            const float* src = rowp[sr];
            const float rs = rscale[sr];
            half_t* dst = w.data() + (size_t)pr * K;
            if (ln_gamma) {      // LayerNorm folded into this Linear: W' = fp16(gamma_k W_nk), u = sum_k W', bias += sum_k beta_k W_nk
                double us = 0.0, cs = 0.0;
                for (int k = 0; k < K; ++k) {
                    dst[k] = (half_t)(src[k] * rs * ln_gamma[k]);
                    us += (double)(float)dst[k];
                    cs += (double)ln_beta[k] * (double)(src[k] * rs);
                }
                lnu[pr] = (float)us;
                bias[pr] = (float)((double)(bflat[sr] * rs) + cs);
                continue;
            }
            if (kmap.empty()) for (int k = 0; k < K; ++k) dst[k] = (half_t)(src[k] * rs);
            else for (int k = 0; k < K; ++k) if (kmap[k] >= 0) dst[k] = (half_t)(src[kmap[k]] * rs);
            bias[pr] = bflat[sr] * rs;
        }
        g.N = N; g.K = K; g.k_real = K_src;
        g.w = upload(w, g.w);
        g.bias = upload(bias, g.bias);
        g.ln_u = ln_gamma ? upload(lnu, g.ln_u) : nullptr;
        if (ln_gamma && !kmap.empty()) return fail(FGDM_ERR_ARG, "LayerNorm fold: plain Linear weights only");
        return (g.w && g.bias && (!ln_gamma || g.ln_u)) ? FGDM_OK : fail(FGDM_ERR_NOMEM, "hipMalloc failed while packing weights");
    }
    // ln: state-dict prefix of the LayerNorm whose output feeds this Linear (folded in, see IgemmArgs::ln_stats)
    int pack_linear(GemmW& g, const std::string& pre, bool has_bias, bool geglu = false, float wscale = 1.f,
                    const std::string& ln = std::string()) {
        const ParamSlot* w = slot(pre + ".weight");
        if (!w) return FGDM_ERR_STATE;
        const ParamSlot *lg = nullptr, *lb = nullptr;
        if (!ln.empty()) { lg = slot(ln + ".weight"); lb = slot(ln + ".bias"); if (!lg || !lb) return FGDM_ERR_STATE; }
        const ParamSlot* b = has_bias ? slot(pre + ".bias") : nullptr;
        if (has_bias && !b) return FGDM_ERR_STATE;
        const int N = (int)w->shape[0], K = (int)(w->numel() / w->shape[0]);
        if (K & 63) return fail(FGDM_ERR_ARG, "linear K not a multiple of 64: " + pre);
        if (lg && (int)lg->numel() != K) return fail(FGDM_ERR_ARG, "LayerNorm fold: width mismatch for " + pre);
        return pack_rows(g, {{w->host.data(), N}}, K, K, {}, {b ? b->host.data() : nullptr}, geglu, {wscale},
                         lg ? lg->host.data() : nullptr, lb ? lb->host.data() : nullptr);
    }
    int pack_stack(GemmW& g, const std::vector<std::string>& pres, bool has_bias, const std::vector<float>& scales = {},
                   const std::string& ln = std::string()) {
        const ParamSlot *lg = nullptr, *lb = nullptr;
        if (!ln.empty()) { lg = slot(ln + ".weight"); lb = slot(ln + ".bias"); if (!lg || !lb) return FGDM_ERR_STATE; }
        std::vector<std::pair<const float*, int>> srcs;
        std::vector<const float*> biases;
        int K = 0;
        for (auto& pre : pres) {
            const ParamSlot* w = slot(pre + ".weight");
            if (!w) return FGDM_ERR_STATE;
            K = (int)(w->numel() / w->shape[0]);
            srcs.push_back({w->host.data(), (int)w->shape[0]});
            if (has_bias) { const ParamSlot* b = slot(pre + ".bias"); if (!b) return FGDM_ERR_STATE; biases.push_back(b->host.data()); }
        }
        return pack_rows(g, srcs, K, K, {}, biases, false, scales, lg ? lg->host.data() : nullptr, lb ? lb->host.data() : nullptr);
    }
    // conv3x3 [Cout, Cin, 3, 3] -> k = tap * Cin + c (implicit GEMM) or im2col layout with padded Cin / K
    // up: the conv of an Upsample layer -- where the phase form can serve it (igemm_up_phase's geometry) the four summed 2x2 kernels
    // are packed NEXT TO the 3x3 pack (FGDM_IGEMM_UP_PHASE switches between them in one build), from the fp32 weights, rounded once
    int pack_conv3(GemmW& g, const std::string& pre, bool up = false) {
        const ParamSlot* w = slot(pre + ".weight");
        const ParamSlot* b = slot(pre + ".bias");
        if (!w || !b) return FGDM_ERR_STATE;
        const int N = (int)w->shape[0], Cin = (int)w->shape[1];
        int cp = 0;
        const std::vector<int> kmap = conv3_kmap(Cin, &cp);      // source row layout is [Cin][3][3]
        g.im2col = (Cin % 64) != 0;
        g.cin_pad = cp;
        half_t* const wph_now = g.wph;
        g.wph = nullptr;
        if (up && Cin % 64 == 0 && N % 320 == 0) {
            g.wph = upload(up_phase_pack(w->host.data(), N, Cin, igemm_npad(N)), wph_now);
            if (!g.wph) return fail(FGDM_ERR_NOMEM, "hipMalloc failed while packing weights");
        }
        return pack_rows(g, {{w->host.data(), N}}, Cin * 9, (int)kmap.size(), kmap, {b->host.data()}, false);
    }
    int pack_norm(NormW& n, const std::string& pre) {
        const ParamSlot* w = slot(pre + ".weight");
        const ParamSlot* b = slot(pre + ".bias");
        if (!w || !b) return FGDM_ERR_STATE;
        n.C = (int)w->shape[0];
        n.g = upload(w->host, n.g);
        n.b = upload(b->host, n.b);
        return (n.g && n.b) ? FGDM_OK : fail(FGDM_ERR_NOMEM, "hipMalloc failed");
    }
    // fp32 [co][ci] weights of a 1x1 convolution followed by its biases, for the per-pixel kernels (vae_prequant, vae_moments)
    int pack_pointwise(float** dst, const std::string& pre) {
        const ParamSlot* w = slot(pre + ".weight");
        const ParamSlot* b = slot(pre + ".bias");
        if (!w || !b) return FGDM_ERR_STATE;
        std::vector<float> wb(w->host);
        wb.insert(wb.end(), b->host.begin(), b->host.end());
        *dst = upload(wb, *dst);
        return *dst ? FGDM_OK : fail(FGDM_ERR_NOMEM, "hipMalloc failed");
    }
    // fp32 table as it is (CLIP's embeddings)
    int pack_table(float** dst, const std::string& name) {
        const ParamSlot* w = slot(name);
        if (!w) return FGDM_ERR_STATE;
        *dst = upload(w->host, *dst);
        return *dst ? FGDM_OK : fail(FGDM_ERR_NOMEM, "hipMalloc failed");
    }
    // The packing visitor of model.h's traversals: every call lands in one of the pack_* above; after the first failure the rest
    // of the walk does nothing.  What depends on the engine's knobs is decided here, at pack time: ln_fold is read at fgdm_create.
    struct Packer {
        fgdm_engine& e;
        int rc = FGDM_OK;
        template <class F> void run(F pack) { if (rc == FGDM_OK) rc = pack(); }
        // softmax(q k^T d^-1/2) is evaluated as exp2 of (q log2(e) d^-1/2) k^T: the constant is folded into the to_q weights
        // here, in fp32, so the scaled query carries ONE fp16 rounding (attention.py:190-193)
        static float qscale(const LinOpt& o) { return o.q_head_dim ? 1.4426950408889634f / sqrtf((float)o.q_head_dim) : 1.f; }
        // norm1 / norm2 / norm3 are folded into the Linears they feed (no normalised copy of the tokens is ever stored) ...
        std::string fold(const LinOpt& o) const { return e.ln_fold ? o.ln : std::string(); }
        // ... or, FGDM_LN_FOLD=0, packed as norms of their own
        void layernorm(NormW& n, const std::string& pre, int C) { if (!e.ln_fold) norm(n, pre, C); }
        void norm(NormW& n, const std::string& pre, int) { run([&] { return e.pack_norm(n, pre); }); }
        void conv3(GemmW& g, const std::string& pre, int, int) { run([&] { return e.pack_conv3(g, pre); }); }
        void conv3_up(GemmW& g, const std::string& pre, int, int) { run([&] { return e.pack_conv3(g, pre, true); }); }
        void pointwise(float*& dst, const std::string& pre, int, int) { run([&] { return e.pack_pointwise(&dst, pre); }); }
        void table(float*& dst, const std::string& key, int, int) { run([&] { return e.pack_table(&dst, key); }); }
        void source(const std::string&, int, int, bool) {}
        void linear(GemmW& g, const std::string& pre, int, int, bool, bool bias, const LinOpt& o = LinOpt()) {
            run([&] { return e.pack_linear(g, pre, bias, o.geglu, qscale(o), fold(o)); });
        }
        void stack(GemmW& g, const std::vector<std::string>& pres, bool bias, const LinOpt& o = LinOpt()) {
            run([&] { return e.pack_stack(g, pres, bias, o.q_head_dim ? std::vector<float>{qscale(o)} : std::vector<float>(), fold(o)); });
        }
    };
    // (re)pack one component if it was never packed or tensors of it were loaded since: the old packed copy is freed, the
    // component's traversal (model.h) is run with the Packer, and the host staging is released
    int repack(int c) {
        Component& comp = comps[c];
        if (comp.packed && !comp.dirty) return FGDM_OK;
        for (auto& name : order) {
            const ParamSlot& ps = params[name];
            if (ps.comp == c && ps.loaded && ps.host.empty())
                return fail(FGDM_ERR_STATE, "tensor " + name + " was released after packing: reload every tensor of " + comp.prefix +
                                            " before finalizing again");
        }
        drop_snapshot();            // it holds copies of buffers that are freed here
        for (void* p : comp.allocs) { (void)hipFree(p); alloc_bytes.erase(p); }
        comp.allocs.clear();
        cur_comp = c;
        Packer pk{*this};
        visit_component(c, pk);
        cur_comp = -1;
        if (pk.rc != FGDM_OK) return pk.rc;
        for (auto& name : order) { ParamSlot& ps = params[name]; if (ps.comp == c) std::vector<float>().swap(ps.host); }
        comp.packed = true;
        comp.dirty = false;
        return FGDM_OK;
    }

    // ------------------------------------------------------------------------------------ weight updates of a finalized engine
    void drop_snapshot() {
        for (auto& sn : snap) (void)hipFree(sn.copy);
        snap.clear();
    }
    size_t snapshot_bytes() const { size_t n = 0; for (auto& sn : snap) n += sn.bytes; return n; }
    // everything computed from weights and kept across calls: the registered context's K / V^T, the summed adapter features, the
    // ControlNets' hint-block outputs.  Their owners set them again (a call that needs one and finds none is refused by name).
    void drop_derived() {
        drop_context();
        drop_adapter_conds();
        for (auto& n : cns) if (n.guided.p) { (void)hipFree(n.guided.p); n.guided = Tensor{}; }
    }
    // the visitor that lists the device buffers of the units it is shown
    struct Collector {
        std::vector<void*> ptrs;
        void add(void* p) { if (p) ptrs.push_back(p); }
        void gemm(GemmW& g) { add(g.w); add(g.bias); add(g.ln_u); add(g.wph); }
        void norm(NormW& n, const std::string&, int) { add(n.g); add(n.b); }
        void layernorm(NormW& n, const std::string& pre, int C) { norm(n, pre, C); }
        void conv3(GemmW& g, const std::string&, int, int) { gemm(g); }
        void conv3_up(GemmW& g, const std::string&, int, int) { gemm(g); }
        void pointwise(float*& d, const std::string&, int, int) { add(d); }
        void table(float*& d, const std::string&, int, int) { add(d); }
        void linear(GemmW& g, const std::string&, int, int, bool, bool, const LinOpt& = LinOpt()) { gemm(g); }
        void stack(GemmW& g, const std::vector<std::string>&, bool, const LinOpt& = LinOpt()) { gemm(g); }
    };
    static bool any_of_keys(const Keys& keys, const std::function<bool(const std::string&)>& has) {
        for (auto& k : keys) if (has(k)) return true;
        return false;
    }
    int weights_snapshot(const char* const* keys, int n) {
        if (!finalized) return fail(FGDM_ERR_STATE, "weights not finalized");
        std::unordered_map<std::string, int> want;
        for (int i = 0; i < n; ++i) {
            if (!keys[i] || !params.count(keys[i])) return fail(FGDM_ERR_ARG, std::string("unknown parameter key: ") + (keys[i] ? keys[i] : "(null)"));
            want[keys[i]] = 1;
        }
        Collector col;
        visit_units(ln_fold, [&](const Keys& unit, auto&& replay) {
            if (any_of_keys(unit, [&](const std::string& k) { return want.count(k) != 0; })) replay(col);
        });
        (void)hipDeviceSynchronize();      // no packed buffer is being written: updates and restores are synchronous
        const size_t had = snap.size();
        for (void* p : col.ptrs) {
            bool held = false;
            for (auto& sn : snap) held = held || sn.dst == p;
            if (held) continue;             // the bytes kept are the ones from before the FIRST update
            Snap sn{p, nullptr, alloc_bytes.at(p)};
            if (hipMalloc(&sn.copy, sn.bytes) != hipSuccess || hipMemcpy(sn.copy, p, sn.bytes, hipMemcpyDeviceToDevice) != hipSuccess) {
                (void)hipFree(sn.copy);
                for (size_t i = had; i < snap.size(); ++i) (void)hipFree(snap[i].copy);
                snap.resize(had);
                return fail(FGDM_ERR_NOMEM, "hipMalloc (weight snapshot)");
            }
            snap.push_back(sn);
        }
        return FGDM_OK;
    }
    int weights_restore(hipStream_t st) {
        if (!finalized) return fail(FGDM_ERR_STATE, "weights not finalized");
        if (snap.empty()) return fail(FGDM_ERR_STATE, "no weight snapshot to restore (fgdm_weights_snapshot)");
        if (hipStreamSynchronize(st) != hipSuccess) return fail(FGDM_ERR_HIP, "hipStreamSynchronize");      // launches still reading the weights
        for (auto& sn : snap)
            if (hipMemcpy(sn.dst, sn.copy, sn.bytes, hipMemcpyDeviceToDevice) != hipSuccess) return fail(FGDM_ERR_HIP, "hipMemcpy (weight restore)");
        (void)hipDeviceSynchronize();
        drop_snapshot();
        drop_derived();
        return FGDM_OK;
    }
    int weights_update_tensor(const char* key, const float* dev, const int64_t* shape, int ndim) {
        if (!finalized) return fail(FGDM_ERR_STATE, "weights not finalized: fgdm_weights_update_tensor changes a packed engine (load with fgdm_load_tensor)");
        if (!upd_open) return fail(FGDM_ERR_STATE, "fgdm_weights_begin_update has not been called");
        auto it = params.find(key);
        if (it == params.end()) return fail(FGDM_ERR_ARG, std::string("unknown parameter key: ") + key);
        const ParamSlot& ps = it->second;
        if ((int)ps.shape.size() != ndim) return fail(FGDM_ERR_ARG, std::string("rank mismatch for ") + key);
        for (int i = 0; i < ndim; ++i)
            if (ps.shape[i] != shape[i]) return fail(FGDM_ERR_ARG, std::string("shape mismatch for ") + key);
        std::vector<float> h(ps.numel());
        if (hipMemcpy(h.data(), dev, h.size() * sizeof(float), hipMemcpyDefault) != hipSuccess) return fail(FGDM_ERR_HIP, "hipMemcpy failed");
        upd[key] = std::move(h);
        return FGDM_OK;
    }
    int weights_commit(hipStream_t st) {
        if (!finalized) return fail(FGDM_ERR_STATE, "weights not finalized");
        if (!upd_open) return fail(FGDM_ERR_STATE, "fgdm_weights_begin_update has not been called");
        upd_open = false;                   // a commit ends the update, refused or not
        std::unordered_map<std::string, std::vector<float>> staged;
        staged.swap(upd);
        auto has = [&](const std::string& k) { return staged.count(k) != 0; };
        for (const Keys& unit : plan_units(ln_fold, has))
            for (auto& k : unit)
                if (!has(k)) return fail(FGDM_ERR_ARG, "partly supplied packed layer: " + k + " is packed together with " +
                                                       *std::find_if(unit.begin(), unit.end(), has) + " and was not supplied");
        if (staged.empty()) return FGDM_OK;
        if (hipStreamSynchronize(st) != hipSuccess) return fail(FGDM_ERR_HIP, "hipStreamSynchronize");      // launches still reading the weights
        for (auto& kv : staged) params[kv.first].host.swap(kv.second);
        Packer pk{*this};
        in_place = true;
        visit_units(ln_fold, [&](const Keys& unit, auto&& replay) { if (any_of_keys(unit, has)) replay(pk); });
        in_place = false;
        for (auto& kv : staged) std::vector<float>().swap(params[kv.first].host);
        (void)hipDeviceSynchronize();
        drop_derived();
        if (pk.rc == FGDM_ERR_NOMEM) return fail(FGDM_ERR_HIP, "writing the re-packed weights failed");
        return pk.rc;
    }

#define CHK(x) do { int _rc = (x); if (_rc != FGDM_OK) return _rc; } while (0)
    // ------------------------------------------------------------------------------------ runtime helpers
    // device-to-device copy / memset on the call's stream, deferred like every launch while a walk is being recorded
    int dcopy(void* dst, const void* src, size_t bytes) {
        auto run = [=](hipStream_t rs) -> int { return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, rs) == hipSuccess ? FGDM_OK : FGDM_ERR_HIP; };
        if (!fgdm_recording()) return run(s);
        fgdm_record(run);
        return FGDM_OK;
    }
    int dzero(void* dst, size_t bytes) {
        auto run = [=](hipStream_t rs) -> int { return hipMemsetAsync(dst, 0, bytes, rs) == hipSuccess ? FGDM_OK : FGDM_ERR_HIP; };
        if (!fgdm_recording()) return run(s);
        fgdm_record(run);
        return FGDM_OK;
    }
    // A new block of `ar` into *t (empty before: assigning over a live handle would release it AFTER the new block was taken)
    int talloc(Act* t, int B, int H, int W, int C, const char* what = "workspace") {
        Tensor v; v.B = B; v.H = H; v.W = W; v.C = C;
        v.p = (half_t*)ar->alloc(v.numel() * sizeof(half_t));
        *t = Act(v, ar);
        return v.p ? FGDM_OK : fail(FGDM_ERR_NOMEM, what);
    }
    int balloc(Buf* b, size_t bytes) {
        *b = Buf(Raw{ar->alloc(bytes)}, ar);
        return b->p ? FGDM_OK : fail(FGDM_ERR_NOMEM, "workspace");
    }

    // LayerNorm partial sums of a token matrix (IgemmArgs::stats_out / ln_stats): [rows][slots][2] floats in the arena
    struct LnView { float* p = nullptr; int slots = 0; };
    using LnStats = Owned<LnView>;
    struct Epi {
        const LnStats* ln = nullptr;   // the A operand is to be LayerNorm-ed: the weights have it folded in (GemmW::ln_u)
        LnStats* stats = nullptr;      // also produce the partial sums of the OUTPUT rows (for the next folded LayerNorm)
        int act = ACT_NONE;
        const float* rowvec = nullptr; int rv_stride = 0;
        const half_t* resid = nullptr; int ld_res = 0;
        float scale = 1.f;
        int out_kind = OUT_F16;
        void* out = nullptr;   // override destination (OUT_F32* kinds or in-place adds)
        int ld_out = 0;
        void* out2 = nullptr; int out_kind2 = OUT_F16, ld_out2 = 0, split_n = 0;   // second destination (IgemmArgs::out2)
        int rps = 0;           // rows per sample override
    };
    // out = epilogue(A W^T): LINEAR over rows of x0 (x1 = virtual concat), or conv3x3 in `mode`
    int gemm(const GemmW& w, int mode, const Tensor& x0, const Tensor* x1, int Ho, int Wo, const Epi& e, Tensor* out) {
        IgemmArgs a{};
        a.A0 = x0.p; a.C0 = x0.C;
        a.A1 = x1 ? x1->p : nullptr; a.C1 = x1 ? x1->C : 0;
        a.Wt = w.w; a.bias = w.bias;
        a.rowvec = e.rowvec; a.rv_stride = e.rv_stride;
        a.resid = e.resid; a.ld_res = e.ld_res;
        a.zero = zero;
        a.B = x0.B; a.H = x0.H; a.W = x0.W; a.Ho = Ho; a.Wo = Wo;
        a.M = x0.B * Ho * Wo;
        a.N = w.N;
        a.K = w.K;
        a.mode = mode; a.act = e.act; a.out_kind = e.out_kind;
        const int nout = e.act == ACT_GEGLU ? w.N / 2 : w.N;
        a.out = e.out ? e.out : (void*)out->p;
        a.ld_out = e.ld_out ? e.ld_out : nout;
        a.rows_per_sample = e.rps ? e.rps : Ho * Wo;
        a.scale = e.scale;
        a.out2 = e.out2; a.out_kind2 = e.out_kind2; a.ld_out2 = e.ld_out2; a.split_n = e.split_n;
        const int taps = mode == IG_LINEAR ? 1 : 9;
        if (taps * (a.C0 + a.C1) != a.K) return fail(FGDM_ERR_ARG, "gemm: K mismatch");
        if (!a.out) return fail(FGDM_ERR_NOMEM, "gemm: null output (workspace exhausted?)");
        // an Upsample conv whose geometry the phase form serves (and whose phase kernels were packed) runs as four 2x2 phase GEMMs
        if (w.wph && !e.stats && !e.ln && igemm_up_phase(a)) a = igemm_phase_args(a, w.wph);
        char tag[56] = "";
        // (l: LayerNorm folded in, s: emits LayerNorm partial sums, r: residual, v: per-sample emb row)
        if (prof.on) snprintf(tag, sizeof(tag), "igemm M%d N%d K%d mode%d act%d out%d l%ds%dr%dv%d", a.M, a.N, a.K, a.mode, a.act, a.out_kind,
                              e.ln ? 1 : 0, e.stats ? 1 : 0, e.resid ? 1 : 0, e.rowvec ? 1 : 0);
        a.splitk = igemm_splitk_factor(a);
        Buf ws;
        if (a.splitk > 1) {
            ws = Buf(Raw{ar->alloc((size_t)a.splitk * a.M * a.N * sizeof(float))}, ar);
            if (!ws.p) return fail(FGDM_ERR_NOMEM, "workspace (split-K partials)");
            a.ws = ws.as<float>();
        }
        if (e.ln) {
            if (!w.ln_u || !e.ln->p || a.splitk > 1) return fail(FGDM_ERR_STATE, "gemm: LayerNorm fold without folded weights / statistics");
            a.ln_stats = e.ln->p; a.ln_slots = e.ln->slots; a.ln_u = w.ln_u; a.ln_eps = w.ln_eps;
        } else if (w.ln_u) {
            return fail(FGDM_ERR_STATE, "gemm: these weights have a LayerNorm folded in; statistics are required");
        }
        if (e.stats) {     // partial sums of the output rows: from the GEMM's own epilogue when its kernel can, else one more pass
            const int slots = igemm_stats_slots(a);
            *e.stats = LnStats(LnView{(float*)ar->alloc((size_t)a.M * std::max(slots, row_stats_slots(nout)) * 2 * sizeof(float)), slots}, ar);
            if (!e.stats->p) return fail(FGDM_ERR_NOMEM, "workspace (LayerNorm statistics)");
            if (e.stats->slots) a.stats_out = e.stats->p;
        }
        double nbytes = 0.0;
        if (prof.on) {      // operands once: activations + weights + residual + output
            const double in_b = 2.0 * ((double)x0.numel() + (x1 ? (double)x1->numel() : 0.0));
            const double out_b = (double)a.M * nout * (e.out_kind == OUT_F16 || e.out_kind == OUT_F16_T ? 2.0 : 4.0);
            nbytes = in_b + 2.0 * (double)w.N * w.K + out_b + (e.resid ? 2.0 * (double)a.M * nout : 0.0);
        }
        prof.begin(PC_IGEMM, s, 2.0 * (double)x0.B * Ho * Wo * (double)w.N * (double)w.k_real, tag, nbytes);    // (algorithmic flops)
        int rc = igemm_launch(a, s);
        prof.end(s);
        ws.reset();
        if (rc == FGDM_OK && e.stats && e.stats->slots == 0) {
            if (a.out_kind != OUT_F16 || a.ld_out != nout) return fail(FGDM_ERR_ARG, "gemm: row statistics need a dense fp16 output");
            e.stats->slots = row_stats_slots(nout);
            prof.begin(PC_NORM, s, 2.0 * (double)a.M * nout, "row_stats");
            rc = row_stats_launch((const half_t*)a.out, a.M, nout, e.stats->p, s);
            prof.end(s);
        }
        return rc == FGDM_OK ? rc : fail(rc, "igemm launch failed");
    }
    // conv3x3 (stride 1/2, FGDM_STRIDE2_PAD_BR, or on the nearest-2x upsampled input) -> new tensor
    int conv3(const GemmW& w, const Tensor& x, const Tensor* x1, int stride, bool up, Epi e, Act* out) {
        int Ho = x.H, Wo = x.W, mode = IG_CONV3;
        if (up) { Ho *= 2; Wo *= 2; mode = IG_CONV3_UP2; }
        else if (stride == 2) { Ho = (x.H - 1) / 2 + 1; Wo = (x.W - 1) / 2 + 1; mode = IG_CONV3_S2; }
        else if (stride == FGDM_STRIDE2_PAD_BR) { Ho = (x.H - 2) / 2 + 1; Wo = (x.W - 2) / 2 + 1; mode = IG_CONV3_S2_BR; }
        if (!e.out) CHK(talloc(out, x.B, Ho, Wo, w.N));
        if (!w.im2col) return gemm(w, mode, x, x1, Ho, Wo, e, out);
        if (up || x1 || x.C != w.cin_pad || stride == FGDM_STRIDE2_PAD_BR) return fail(FGDM_ERR_ARG, "im2col conv path: unsupported combination");
        Act A;
        CHK(talloc(&A, 1, 1, x.B * Ho * Wo, w.K, "workspace (im2col)"));
        prof.begin(PC_ELEM, s, 2.0 * (double)A.numel() + 2.0 * (double)x.numel());
        bool in_gemm = false;
        const int rc = im2col_conv(x.p, A.p, x.B, x.H, x.W, x.C, stride, w.K, s, [&]() { prof.end(s); },
            [&](half_t* Ap, int Bv, int Hv, int Wv, int Kv, int rps) {
                in_gemm = true;
                Tensor Av; Av.p = Ap; Av.B = Bv; Av.H = Hv; Av.W = Wv; Av.C = Kv;
                if (!e.rps) e.rps = rps;
                return gemm(w, IG_LINEAR, Av, nullptr, Hv, Wv, e, out);
            });
        return rc != FGDM_OK && !in_gemm ? fail(rc, "im2col failed") : rc;
    }
    int linear(const GemmW& w, const Tensor& x, Epi e, Act* out, const Tensor* x1 = nullptr) {
        if (!e.out) CHK(talloc(out, x.B, x.H, x.W, e.act == ACT_GEGLU ? w.N / 2 : w.N));
        return gemm(w, IG_LINEAR, x, x1, x.H, x.W, e, out);
    }
    int gnorm(const NormW& n, const Tensor& x, const Tensor* x1, float eps, bool silu, Act* out) {
        const int C = x.C + (x1 ? x1->C : 0);
        Buf ws;
        CHK(talloc(out, x.B, x.H, x.W, C));
        CHK(balloc(&ws, groupnorm_ws_floats(x.B, x.H * x.W) * sizeof(float)));
        char tag[56] = "";
        if (prof.on) snprintf(tag, sizeof(tag), "groupnorm B%d HW%d C%d", x.B, x.H * x.W, C);
        prof.begin(PC_NORM, s, 4.0 * (double)out->numel(), tag);   // algorithmic: read once + write once, fp16
        const int rc = groupnorm_launch(x.p, x.C, x1 ? x1->p : nullptr, x1 ? x1->C : 0, x.B, x.H * x.W, n.g, n.b, eps,
                                        silu ? 1 : 0, out->p, ws.as<float>(), s);
        prof.end(s);
        return rc == FGDM_OK ? rc : fail(rc, "groupnorm launch failed");
    }
    int lnorm(const NormW& n, const Tensor& x, Act* out) {
        CHK(talloc(out, x.B, x.H, x.W, x.C));
        char tag[56] = "";
        if (prof.on) snprintf(tag, sizeof(tag), "layernorm rows%d C%d", x.rows(), x.C);
        prof.begin(PC_NORM, s, 4.0 * (double)out->numel(), tag);
        const int rc = layernorm_launch(x.p, x.rows(), x.C, n.g, n.b, 1e-5f, out->p, s);
        prof.end(s);
        return rc == FGDM_OK ? rc : fail(rc, "layernorm launch failed");
    }

    // ------------------------------------------------------------------------------------ layers
    struct EmbCtx { const float* emb_all; int stride; };

    // ResBlock._forward (openaimodel.py:275-301); x1 = skip tensor of the decoder's channel concat.  Also the first stage's
    // ResnetBlock.forward with temb = None (model.py:121-141): no timestep row, GroupNorm eps 1e-6
    int res_fwd(const Layer& l, const Tensor& x, const Tensor* x1, const EmbCtx& ec, Act* out) {
        Act g1, h, g2, sk, xp;
        CHK(gnorm(l.gn1, x, x1, l.eps, true, &g1));
        const Tensor* xs = &x;       // the tensor the skip path reads
        if (l.down) {                // ResBlock(down=True, use_conv=False): AvgPool2d(2) on h and on x (openaimodel.py:276-282)
            if (x1) return fail(FGDM_ERR_ARG, "down ResBlock with a concatenated input");
            Act gp;
            CHK(talloc(&gp, x.B, x.H / 2, x.W / 2, x.C));
            CHK(talloc(&xp, x.B, x.H / 2, x.W / 2, x.C));
            if (avgpool2(g1.p, gp.p, x.B, x.H, x.W, x.C, s) != FGDM_OK || avgpool2(x.p, xp.p, x.B, x.H, x.W, x.C, s) != FGDM_OK)
                return fail(FGDM_ERR_ARG, "avgpool2: latent size must be divisible by 8 for the adapter");
            g1 = std::move(gp);
            xs = &xp;
        }
        Epi e1;
        if (l.emb_off >= 0) { e1.rowvec = ec.emb_all + l.emb_off; e1.rv_stride = ec.stride; }
        CHK(conv3(l.c1, g1, nullptr, 1, false, e1, &h));
        g1.reset();
        CHK(gnorm(l.gn2, h, nullptr, l.eps, true, &g2));
        h.reset();
        Epi e2;
        if (l.cin != l.cout) {
            CHK(linear(l.skip, *xs, Epi{}, &sk, x1));
            e2.resid = sk.p; e2.ld_res = sk.C;
        } else {
            e2.resid = xs->p; e2.ld_res = xs->C;
        }
        return conv3(l.c2, g2, nullptr, 1, false, e2, out);      // g2, sk and xp go back behind it
    }

    // attn2's k = to_k(context), v = to_v(context) (attention.py:183-186); V is produced transposed for the kernel.
    // persistent = true: buffers come from hipMalloc and live in ctx_cache until the next set_context (the handles own nothing)
    int cross_kv(const Layer& l, const Tensor& ctx16, bool persistent, Act* k2, Act* v2t) {
        const int B = ctx16.B, C = l.cin, Tk = ctx16.H * ctx16.W, Tkp = roundup(Tk, 64);
        if (persistent) {
            k2->B = B; k2->H = ctx16.H; k2->W = ctx16.W; k2->C = C;
            v2t->B = B; v2t->H = 1; v2t->W = C; v2t->C = Tkp;
            if (hipMalloc(&k2->p, k2->numel() * sizeof(half_t)) != hipSuccess ||
                hipMalloc(&v2t->p, v2t->numel() * sizeof(half_t)) != hipSuccess) return fail(FGDM_ERR_NOMEM, "hipMalloc (context cache)");
            { Epi e; e.out = k2->p; e.ld_out = C; CHK(linear(l.k2, ctx16, e, nullptr)); }
        } else {
            CHK(linear(l.k2, ctx16, Epi{}, k2));
            CHK(talloc(v2t, B, 1, C, Tkp));
        }
        if (Tkp != Tk) CHK(dzero(v2t->p, v2t->numel() * sizeof(half_t)));
        { Epi e; e.out_kind = OUT_F16_T; e.out = v2t->p; e.ld_out = Tkp; e.rps = Tk; CHK(linear(l.v2, ctx16, e, nullptr)); }
        return FGDM_OK;
    }
    void drop_context() {
        for (auto& kv : ctx_cache) { (void)hipFree(kv.second.k.p); (void)hipFree(kv.second.vt.p); }
        ctx_cache.clear();
        ctx_B = 0;
    }
    // The conditioning is the same tensor in every denoising step (ddim.py:147-162 passes `cond` unchanged): project it
    // through every cross-attention layer's to_k / to_v once; apply_model(ctx = NULL) then reuses the projections.
    int set_context(const float* ctx, int B) {
        if (!finalized) return fail(FGDM_ERR_STATE, "weights not finalized");
        if (B <= 0) return fail(FGDM_ERR_ARG, "bad shape");
        drop_context();
        Act ctx16;
        CHK(talloc(&ctx16, B, 1, ctx_tokens, cfg.context_dim));
        if (f32_to_f16(ctx, ctx16.p, ctx16.numel(), s) != FGDM_OK) return fail(FGDM_ERR_HIP, "convert kernel");
        auto walk = [&](const Block& blk) -> int {
            for (const Layer& l : blk)
                if (l.type == L_ATTN) { Act k, vt; CHK(cross_kv(l, ctx16, true, &k, &vt)); ctx_cache[&l] = CtxKV{k, vt}; }
            return FGDM_OK;
        };
        CHK(for_each_block(unet, false, walk));
        for (auto& n : cns) CHK(for_each_block(n, false, walk));
        ctx_B = B; ctx_T = ctx_tokens;
        return FGDM_OK;
    }

    // SpatialTransformer.forward with one BasicTransformerBlock (attention.py:234-292)
    // dup: x holds the SHARED half of a CFG batch (rows b and b + B/2 identical so far); the self-attention part runs on
    // it once, the result is duplicated where the (per-half) context enters, and `out` has 2 * x.B rows
    int attn_fwd(const Layer& l, const Tensor& x_in, const Tensor& ctx16, Act* out, bool dup = false) {
        Tensor x = x_in;
        int B = x.B;
        const int T = x.H * x.W, C = x.C, d = C / l.heads;
        Act g, h, qk, vt, a, h2, q2, k2, v2t, f, x_full;
        LnStats s1, s2, s3;      // row sums of h / h2 / h3 for norm1 / norm2 / norm3, which live inside the next GEMMs
        CHK(gnorm(l.gn, x, nullptr, 1e-6f, false, &g));
        Act nrm;                    // FGDM_LN_FOLD=0 only: the normalised tokens as a tensor of their own
        { Epi e; if (ln_fold) e.stats = &s1; CHK(linear(l.pin, g, e, &h)); }
        g.reset();
        // --- attn1 (self): q | k and v^T straight from h, norm1 folded into both projections
        if (!ln_fold) CHK(lnorm(l.ln1, h, &nrm));
        const Tensor& a1 = ln_fold ? h : nrm;
        // ONE GEMM for to_q | to_k | to_v: q | k row-major [M, 2C], v transposed [B, C, Tp] (the attention kernel's PV operand)
        const int Tp = roundup(T, 64);
        CHK(talloc(&qk, B, x.H, x.W, 2 * C));
        CHK(talloc(&vt, B, 1, C, Tp));
        if (Tp != T) CHK(dzero(vt.p, vt.numel() * sizeof(half_t)));
        { Epi e; if (ln_fold) e.ln = &s1; e.out = qk.p; e.ld_out = 2 * C; e.rps = T;
          e.out2 = vt.p; e.out_kind2 = OUT_F16_T; e.ld_out2 = Tp; e.split_n = 2 * C;
          CHK(linear(l.qkv1, a1, e, nullptr)); }
        s1.reset(); nrm.reset();
        CHK(talloc(&a, B, x.H, x.W, C));
        { char tag[56]; snprintf(tag, sizeof(tag), "attn B%d T%d Tk%d d%d", B, T, T, d);
          prof.begin(PC_ATTN, s, 4.0 * (double)B * T * (double)T * C, tag);
          int rc = attention_launch(qk.p, 2 * C, qk.p + C, 2 * C, vt.p, Tp, a.p, C, B, l.heads, T, T, d, 1, s);
          prof.end(s);
          if (rc != FGDM_OK) return fail(rc, "attention launch failed (unsupported head dim?)"); }
        qk.reset(); vt.reset();
        { Epi e; e.resid = h.p; e.ld_res = C; if (ln_fold) e.stats = &s2; CHK(linear(l.o1, a, e, &h2)); }
        a.reset(); h.reset();
        if (dup) {     // from here on the two halves differ (their contexts do)
            Act f2;
            CHK(dup_rows(h2, &f2)); h2 = std::move(f2);
            CHK(dup_rows(x, &x_full)); x = x_full;
            B *= 2;
        }
        if (dup && ln_fold) {
            const size_t sb = (size_t)(B / 2) * T * s2.slots * 2 * sizeof(float);
            LnStats s2f(LnView{(float*)ar->alloc(2 * sb), s2.slots}, ar);
            if (!s2f.p) return fail(FGDM_ERR_NOMEM, "workspace");
            CHK(dcopy(s2f.p, s2.p, sb));
            CHK(dcopy((char*)s2f.p + sb, s2.p, sb));
            s2 = std::move(s2f);
        }
        // --- attn2 (cross, ctx_tokens-token context), norm2 folded into to_q
        if (!ln_fold) CHK(lnorm(l.ln2, h2, &nrm));
        { Epi e; if (ln_fold) e.ln = &s2; CHK(linear(l.q2, ln_fold ? h2 : nrm, e, &q2)); }
        s2.reset(); nrm.reset();
        int Tk, Tkp;
        const bool cached = (ctx16.p == nullptr);
        if (cached) {      // K / V^T were projected once by set_context
            auto it = ctx_cache.find(&l);
            if (it == ctx_cache.end() || ctx_B != B) return fail(FGDM_ERR_STATE, "no cached context for this batch (fgdm_set_context)");
            k2 = borrow(it->second.k); v2t = borrow(it->second.vt);
            Tk = ctx_T; Tkp = roundup(Tk, 64);
        } else {
            Tk = ctx16.H * ctx16.W; Tkp = roundup(Tk, 64);
            CHK(cross_kv(l, ctx16, false, &k2, &v2t));
        }
        CHK(talloc(&a, B, x.H, x.W, C));
        { char tag[56]; snprintf(tag, sizeof(tag), "attn B%d T%d Tk%d d%d", B, T, Tk, d);
          prof.begin(PC_ATTN, s, 4.0 * (double)B * T * (double)Tk * C, tag);
          int rc;
          auto cp = cap.capturing ? cap.planes.find(&l) : cap.planes.end();
          if (cp != cap.planes.end()) {      // a selected UNet block: the capturing instantiation, then the head reduction into its accumulator
              const CapPlane& p = cp->second;
              if (B != cap.B || T != p.h * p.w || Tk != cap.Tk) return fail(FGDM_ERR_STATE, "attention capture: block shape differs from the plan's");
              rc = attention_capture_launch(q2.p, C, k2.p, C, v2t.p, Tkp, a.p, C, B, l.heads, T, Tk, d, 1, cap.head_planes, s);
              if (rc == FGDM_OK)
                  rc = attention_maps_reduce(cap.head_planes, p.acc, l.heads, T, Tk, cap.row0, cap.rows, cap.tok_dev, (int)cap.tokens.size(),
                                             cap.mode == FGDM_CAPTURE_SUM, s);
          } else {
              rc = attention_launch(q2.p, C, k2.p, C, v2t.p, Tkp, a.p, C, B, l.heads, T, Tk, d, 1, s);
          }
          prof.end(s);
          if (rc != FGDM_OK) return fail(rc, "attention launch failed"); }
        q2.reset(); k2.reset(); v2t.reset();      // (a cached K / V^T was only borrowed)
        { Epi e; e.resid = h2.p; e.ld_res = C; if (ln_fold) e.stats = &s3; CHK(linear(l.o2, a, e, &h)); }
        a.reset(); h2.reset();
        // --- GEGLU feed-forward, norm3 folded into the projection
        if (!ln_fold) CHK(lnorm(l.ln3, h, &nrm));
        { Epi e; if (ln_fold) e.ln = &s3; e.act = ACT_GEGLU; CHK(linear(l.ffp, ln_fold ? h : nrm, e, &f)); }
        s3.reset(); nrm.reset();
        { Epi e; e.resid = h.p; e.ld_res = C; CHK(linear(l.ffo, f, e, &h2)); }
        f.reset(); h.reset();
        Epi e; e.resid = x.p; e.ld_res = C;
        return linear(l.pout, h2, e, out);      // h2 and x_full go back behind it
    }

    // [x] -> [x; x]: the two halves of a classifier-free-guidance batch share everything up to the first cross-attention
    int dup_rows(const Tensor& h, Act* full) {
        CHK(talloc(full, 2 * h.B, h.H, h.W, h.C));
        const size_t bytes = h.numel() * sizeof(half_t);
        CHK(dcopy(full->p, h.p, bytes));
        CHK(dcopy((char*)full->p + bytes, h.p, bytes));
        return FGDM_OK;
    }

    // TimestepEmbedSequential over one block; x1 = decoder skip (consumed by the block's first ResBlock).  x is consumed: it goes
    // back to its arena as soon as the first layer has read it -- unless the caller only lent it (borrow()).
    // shared: x holds the SHARED half of a CFG batch (FGDM_FLAG_CFG_PAIRS): the layers run on B/2 rows until the context enters
    // (attn2 of the first SpatialTransformer); the output has the full 2 * (B/2) rows.
    int block_fwd(const Block& blk, Act x, const Tensor* x1, const EmbCtx& ec, const Tensor& ctx16, const half_t* conv_resid, Act* out,
                  bool shared = false) {
        Act cur = std::move(x);
        bool full = !shared;
        for (size_t j = 0; j < blk.size(); ++j) {
            const Layer& l = blk[j];
            Act nxt;
            switch (l.type) {
                case L_CONV: { Epi e; if (conv_resid) { e.resid = conv_resid; e.ld_res = l.cout; }
                               CHK(conv3(l.conv, cur, nullptr, 1, false, e, &nxt)); break; }
                case L_RES: CHK(res_fwd(l, cur, j == 0 ? x1 : nullptr, ec, &nxt)); break;
                case L_ATTN: CHK(attn_fwd(l, cur, ctx16, &nxt, !full)); full = true; break;
                case L_DOWN: CHK(conv3(l.conv, cur, nullptr, 2, false, Epi{}, &nxt)); break;
                case L_UP: CHK(conv3(l.conv, cur, nullptr, 1, true, Epi{}, &nxt)); break;
            }
            cur = std::move(nxt);
        }
        if (!full) { Act f; CHK(dup_rows(cur, &f)); cur = std::move(f); }
        *out = std::move(cur);
        return FGDM_OK;
    }

    // timestep_embedding -> time_embed -> SiLU -> all emb_layers (util.py:160-180; openaimodel.py:537-542,827-828,290)
    int embed(Net& n, const int64_t* t, const float* tf, int B, Buf* emb_all) {
        const int mc = cfg.model_channels;
        Act te, e1, e2;
        CHK(talloc(&te, 1, 1, B, mc));
        if (timestep_embed(t, tf, te.p, B, mc, B, s) != FGDM_OK) return fail(FGDM_ERR_HIP, "timestep_embed");
        { Epi e; e.act = ACT_SILU; e.rps = 1; CHK(linear(n.time0, te, e, &e1)); }
        { Epi e; e.act = ACT_SILU; e.rps = 1; CHK(linear(n.time2, e1, e, &e2)); }   // = SiLU(emb): the only use of emb
        CHK(balloc(emb_all, (size_t)B * n.emb_total * sizeof(float)));
        Epi e; e.out_kind = OUT_F32; e.out = emb_all->p; e.ld_out = n.emb_total; e.rps = 1;
        return linear(n.emb_all, e2, e, nullptr);
    }

    // Adapter.forward (adapter.py:334-346): four feature maps from the (noisy) latent itself.
    // ResnetBlock (adapter.py:301-313, ksize=1, sk=True): [AvgPool2d(2)] -> [conv1x1] -> conv3x3 -> ReLU -> conv1x1 -> +x
    // The running activation is `cur` while it is a temporary; every second block's output is moved into feats[k], which owns it
    // from then on, and `x` -- what the next layer reads -- goes on viewing it there.
    int adapter_fwd(Net& n, const Tensor& x4, Act feats[4]) { return adapter_run(n.ad_conv_in, n.ad_body, x4, feats); }
    int adapter_run(const GemmW& conv_in, const std::vector<AdapterBlk>& body, const Tensor& x4, Act feats[4]) {
        Act cur;
        Tensor x;
        auto next = [&](Act& y) { cur = std::move(y); x = cur; };
        { Act y; CHK(conv3(conv_in, x4, nullptr, 1, false, Epi{}, &y)); next(y); }
        for (size_t k = 0; k < body.size(); ++k) {
            const AdapterBlk& b = body[k];
            if (b.down) {
                Act p;
                CHK(talloc(&p, x.B, x.H / 2, x.W / 2, x.C));
                if (avgpool2(x.p, p.p, x.B, x.H, x.W, x.C, s) != FGDM_OK)
                    return fail(FGDM_ERR_ARG, "avgpool2: latent size must be divisible by 8 for the adapter");
                next(p);
            }
            if (b.ic != b.oc) { Act y; CHK(linear(b.in_conv, x, Epi{}, &y)); next(y); }
            Act h, y;
            { Epi e; e.act = ACT_RELU; CHK(conv3(b.b1, x, nullptr, 1, false, e, &h)); }
            { Epi e; e.resid = x.p; e.ld_res = x.C; CHK(linear(b.b2, h, e, &y)); }
            h.reset();
            next(y);
            if (k % 2 == 1) feats[k / 2] = std::move(cur);   // nums_rb = 2: a feature after every second block
        }
        return FGDM_OK;
    }

    void drop_adapter_conds() {
        for (Tensor& t : unet.xad_sum) { if (t.p) (void)hipFree(t.p); t = Tensor{}; }
        unet.xad_valid = false;
    }
    // AdaptUNetModel.forward's `conds` (openaimodel.py:1288-1291,1301-1305): sum_k adapters[k](conds[k]), kept until replaced
    int set_adapter_conds(const float* const* conds, int nc, int B, int H, int W) {
        if (!finalized) return fail(FGDM_ERR_STATE, "weights not finalized");
        Net& n = unet;
        drop_adapter_conds();
        if (nc == 0) return FGDM_OK;
        if (nc < 0 || nc > (int)n.xad_body.size() || !conds) return fail(FGDM_ERR_ARG, "more conds than extra adapters (n_extra_adapters)");
        if (B <= 0 || (H & 7) || (W & 7)) return fail(FGDM_ERR_ARG, "latent size must be divisible by 8 for the adapter");
        for (int kk = 0; kk < nc; ++kk) {
            Act c4, f[4];
            CHK(talloc(&c4, B, H, W, 4));
            if (nchw_f32_to_nhwc_f16(conds[kk], c4.p, B, 4, H * W, 4, s) != FGDM_OK) return fail(FGDM_ERR_HIP, "layout kernel");
            CHK(adapter_run(n.xad_conv_in[kk], n.xad_body[kk], c4, f));
            for (int i = 0; i < 4; ++i) {
                Tensor& acc = n.xad_sum[i];
                if (kk == 0) {
                    acc = f[i];
                    if (hipMalloc(&acc.p, acc.numel() * sizeof(half_t)) != hipSuccess) return fail(FGDM_ERR_NOMEM, "hipMalloc (adapter cache)");
                    HIP_TRY(hipMemcpyAsync(acc.p, f[i].p, acc.numel() * sizeof(half_t), hipMemcpyDeviceToDevice, s));
                } else if (add_f16(acc.p, f[i].p, acc.p, acc.numel(), s) != FGDM_OK) {
                    return fail(FGDM_ERR_HIP, "add kernel");
                }
            }
        }
        n.xad_valid = true;
        return FGDM_OK;
    }

    // TimeAdapter.forward (adapter.py:405-417): conv_in, then 8 time-conditioned ResBlocks, a feature every second one
    int time_adapter_fwd(Net& n, const Tensor& x4, const EmbCtx& ec, Act feats[4]) {
        Act cur;                 // as in adapter_run
        Tensor x;
        CHK(conv3(n.ad_conv_in, x4, nullptr, 1, false, Epi{}, &cur));
        x = cur;
        for (size_t k = 0; k < n.tad_body.size(); ++k) {
            Act y;
            CHK(res_fwd(n.tad_body[k], x, nullptr, ec, &y));
            cur = std::move(y);
            x = cur;
            if (k % 2 == 1) feats[k / 2] = std::move(cur);
        }
        return FGDM_OK;
    }

    // One TimestepEmbedSequential (or the FG-DM adapter) of the loaded graph, addressed by its state-dict prefix: the
    // block-level parity entry (fgdm_run_block)
    int run_block(const std::string& prefix, const float* x, int C, const float* x_skip, int Cs, const float* emb,
                  const float* ctx, int B, int H, int W, float* out, int64_t cap, int64_t* out_numel) {
        if (!finalized) return fail(FGDM_ERR_STATE, "weights not finalized");
        if (B <= 0 || H <= 0 || W <= 0 || C <= 0) return fail(FGDM_ERR_ARG, "bad shape");
        Net* net = nullptr;
        const Block* blk = nullptr;
        Block single;                // the prefix may also name ONE layer of a block ("...input_blocks.4.1.")
        auto scan = [&](Net& n) {
            for_each_block(n, false, [&](const Block& b) {
                if (blk || b.empty()) return FGDM_OK;
                const std::string& lp = b[0].pre;                       // "<block prefix>0."
                if (lp.size() >= 2 && lp.compare(0, lp.size() - 2, prefix) == 0 && lp.size() - 2 == prefix.size()) { blk = &b; net = &n; }
                return FGDM_OK;
            });
        };
        auto scan1 = [&](Net& n) {
            for_each_block(n, false, [&](const Block& b) {
                for (const Layer& l : b) if (single.empty() && l.pre == prefix) { single.push_back(l); net = &n; }
                return FGDM_OK;
            });
        };
        scan(unet);
        for (auto& n : cns) scan(n);
        if (!blk) {
            scan1(unet);
            for (auto& n : cns) scan1(n);
            if (!single.empty()) blk = &single;
        }
        const bool adapter = !blk && unet.has_adapter && !unet.time_adapter && prefix == unet.prefix + "adapter.";
        if (!blk && !adapter) return fail(FGDM_ERR_ARG, "fgdm_run_block: no such block: " + prefix);
        const int HW = H * W;
        auto emit = [&](const Tensor& t, int64_t& off) -> int {
            if (off + (int64_t)t.numel() > cap) return fail(FGDM_ERR_ARG, "fgdm_run_block: output buffer too small");
            if (nhwc_f16_to_nchw_f32(t.p, out + off, t.B, t.C, t.H * t.W, s) != FGDM_OK) return fail(FGDM_ERR_HIP, "layout kernel");
            off += (int64_t)t.numel();
            return FGDM_OK;
        };
        int64_t off = 0;
        Act xin;
        CHK(talloc(&xin, B, H, W, C));
        if (nchw_f32_to_nhwc_f16(x, xin.p, B, C, HW, C, s) != FGDM_OK) return fail(FGDM_ERR_HIP, "layout kernel");
        if (adapter) {
            if (C != 4) return fail(FGDM_ERR_ARG, "adapter input has 4 channels");
            Act fa[4];
            CHK(adapter_fwd(unet, xin, fa));
            for (int i = 0; i < 4; ++i) CHK(emit(fa[i], off));
            if (out_numel) *out_numel = off;
            return FGDM_OK;
        }
        Act xsk, ctx16;
        if (x_skip) {
            CHK(talloc(&xsk, B, H, W, Cs));
            if (nchw_f32_to_nhwc_f16(x_skip, xsk.p, B, Cs, HW, Cs, s) != FGDM_OK) return fail(FGDM_ERR_HIP, "layout kernel");
        }
        if ((*blk)[0].cin != C + (x_skip ? Cs : 0) || (C & 63) || (x_skip && (Cs & 63)))
            return fail(FGDM_ERR_ARG, "fgdm_run_block: channel count does not match the block");
        bool needs_ctx = false, needs_emb = false;
        for (const Layer& l : *blk) { needs_ctx |= l.type == L_ATTN; needs_emb |= l.type == L_RES; }
        if ((needs_ctx && !ctx) || (needs_emb && !emb)) return fail(FGDM_ERR_ARG, "fgdm_run_block: this block needs ctx / emb");
        if (needs_ctx) {
            CHK(talloc(&ctx16, B, 1, ctx_tokens, cfg.context_dim));
            if (f32_to_f16(ctx, ctx16.p, ctx16.numel(), s) != FGDM_OK) return fail(FGDM_ERR_HIP, "convert kernel");
        }
        Buf emb_all;
        if (needs_emb) {   // emb_layers = SiLU -> Linear on the given `emb` (openaimodel.py:238-244), all ResBlocks in one GEMM
            Act e2;
            CHK(talloc(&e2, 1, 1, B, 4 * cfg.model_channels));
            CHK(balloc(&emb_all, (size_t)B * net->emb_total * sizeof(float)));
            if (silu_f32_to_f16(emb, e2.p, e2.numel(), s) != FGDM_OK) return fail(FGDM_ERR_HIP, "silu kernel");
            Epi e; e.out_kind = OUT_F32; e.out = emb_all.p; e.ld_out = net->emb_total; e.rps = 1;
            CHK(linear(net->emb_all, e2, e, nullptr));
        }
        EmbCtx ec{emb_all.as<float>(), net->emb_total};
        Act y;
        CHK(block_fwd(*blk, borrow(xin), x_skip ? &xsk : nullptr, ec, ctx16, nullptr, &y));
        CHK(emit(y, off));
        if (out_numel) *out_numel = off;
        return FGDM_OK;
    }

    int ensure_device() {
        if (device_ready) return FGDM_OK;
        if (hipSetDevice(device) != hipSuccess) return fail(FGDM_ERR_HIP, "hipSetDevice failed (no GPU?)");
        if (hipMalloc(&zero, 4096) != hipSuccess || hipMemset(zero, 0, 4096) != hipSuccess) return fail(FGDM_ERR_HIP, "hipMalloc failed");
        if (cfg.workspace_bytes > 0) arena.slab_bytes = (size_t)cfg.workspace_bytes;
        device_ready = true;
        return FGDM_OK;
    }

    // dst <- dst + scale (W src + b), in place (cldm.py:40,46,846 fused into the zero-conv's epilogue)
    int zero_conv_into(const GemmW& zw, const Tensor& src, Tensor& dst, float scale) {
        Epi e;
        e.scale = scale;
        if (src.B * 2 == dst.B) {      // shared half: the same residual goes into both halves of the UNet's skip tensor
            for (int half = 0; half < 2; ++half) {
                half_t* d = dst.p + (size_t)half * (dst.numel() / 2);
                e.resid = d; e.ld_res = dst.C; e.out = d; e.ld_out = dst.C;
                CHK(linear(zw, src, e, nullptr));
            }
            return FGDM_OK;
        }
        e.resid = dst.p; e.ld_res = dst.C; e.out = dst.p; e.ld_out = dst.C;
        return linear(zw, src, e, nullptr);
    }

    // While it lives, launches are recorded into `walk` (nullptr: enqueued as usual) and workspaces come from `arena`; whatever
    // path leaves, both are as they were before.
    struct RecordScope {
        fgdm_engine& e;
        Arena* const ar0;
        RecWalk* const rec0;
        RecordScope(fgdm_engine& e_, RecWalk* walk, Arena* arena) : e(e_), ar0(e_.ar), rec0(fgdm_record_into(walk)) { e.ar = arena; }
        ~RecordScope() { e.ar = ar0; fgdm_record_into(rec0); }
        RecordScope(const RecordScope&) = delete;
    };
    // What the GEMMs' tile and split-K choices are told about the layers walked while it lives: they have a same-shape twin in
    // another net (igemm_set_twin_layers), and -- pair_mult > 0 -- their launches will be fused pair_mult at a time
    // (igemm_set_pair_hint; 0 leaves the hint as it is).  Whatever path leaves, both are as they were before.
    bool hint_twins = false;
    int hint_pair = 1;
    struct LayerHints {
        fgdm_engine& e;
        const bool twins0;
        const int pair0;
        LayerHints(fgdm_engine& e_, bool twins, int pair_mult = 0) : e(e_), twins0(e_.hint_twins), pair0(e_.hint_pair) {
            e.set_hints(twins, pair_mult > 0 ? pair_mult : pair0);
        }
        ~LayerHints() { e.set_hints(twins0, pair0); }
        LayerHints(const LayerHints&) = delete;
    };
    void set_hints(bool twins, int pair_mult) {
        igemm_set_twin_layers(hint_twins = twins);
        igemm_set_pair_hint(hint_pair = pair_mult);
    }

    // ControlNet.forward (cldm.py:792-813).  fused = true: every zero-conv output is scaled and ADDED in place into
    // the UNet's skip tensor hs[i] / h_mid (cldm.py:40,46 + :846), so control residuals never hit HBM separately.
    // fused = false: raw residuals are written as fp32 NCHW into out32 (test entry).
    int controlnet_fwd(Net& n, const Tensor& x4, const int64_t* t, const float* tf, const Tensor& ctx16, const float* scales,
                       std::vector<Act>* hs, Act* h_mid, bool only_mid, float* out32, int64_t out_cap, bool pairs = false,
                       std::vector<Deferred>* defer = nullptr) {
        const int B = x4.B;
        LayerHints twins(*this, true);
        // CFG pairs: rows b and b + B/2 carry the same x, t and hint -> input blocks 0 and 1 (up to the first
        // cross-attention) are evaluated once on B/2 rows
        const bool shared = pairs && !out32 && 2 * n.guided.B == B && n.input.size() > 1;
        if (!n.guided.p) return fail(FGDM_ERR_STATE, "fgdm_set_hint has not been called for this ControlNet");
        if (!(n.guided.B == B || 2 * n.guided.B == B) || n.guided.H != x4.H || n.guided.W != x4.W)
            return fail(FGDM_ERR_ARG, "cached hint does not match the batch / latent size");
        Buf emb;
        CHK(embed(n, t, tf, B, &emb));
        EmbCtx ec{emb.as<float>(), n.emb_total};
        // the running activation: `h` owns it until a deferred zero-conv takes it over (it needs the block output later, on the
        // main stream); the next block then only borrows it through `hv`
        Act h;
        Tensor hv;
        auto input = [&]() -> Act { return h.p ? std::move(h) : borrow(hv); };
        int64_t off = 0;
        auto zero_conv = [&](const GemmW& zw, Act& src, int idx) -> int {
            Epi e;
            if (out32) {
                const int64_t cnt = (int64_t)src.numel();
                if (off + cnt > out_cap) return fail(FGDM_ERR_ARG, "fgdm_controlnet: output buffer too small");
                e.out_kind = OUT_F32_NCHW; e.out = out32 + off; e.ld_out = src.H * src.W;
                off += cnt;
                return linear(zw, src, e, nullptr);
            }
            if (idx >= 0 && only_mid) return FGDM_OK;
            e.scale = scales ? scales[idx < 0 ? (int)n.input.size() : idx] : 1.f;
            if (defer) { defer->push_back({&zw, std::move(src), idx, e.scale}); return FGDM_OK; }     // applied by the caller on the main stream
            return zero_conv_into(zw, src, idx < 0 ? *h_mid : (*hs)[idx], e.scale);
        };
        for (size_t i = 0; i < n.input.size(); ++i) {
            Act nxt;
            if (i == 0) {
                // h = conv_in(x) + guided_hint (cldm.py:803-805); a B-sized hint serves both halves of a 2B CFG batch
                const Layer& l = n.input[0][0];
                if (shared) {
                    Tensor xh = x4; xh.B = B / 2;
                    CHK(block_fwd(n.input[0], borrow(xh), nullptr, ec, ctx16, n.guided.p, &nxt));
                } else if (n.guided.B == B) {
                    CHK(block_fwd(n.input[0], borrow(x4), nullptr, ec, ctx16, n.guided.p, &nxt));
                } else {
                    CHK(talloc(&nxt, B, x4.H, x4.W, l.cout));
                    for (int half = 0; half < 2; ++half) {
                        Tensor xs = x4; xs.B = B / 2; xs.p = x4.p + (size_t)half * xs.numel();
                        Epi e; e.resid = n.guided.p; e.ld_res = l.cout;
                        e.out = nxt.p + (size_t)half * (nxt.numel() / 2); e.ld_out = l.cout;
                        CHK(conv3(l.conv, xs, nullptr, 1, false, e, nullptr));
                    }
                }
            } else {
                CHK(block_fwd(n.input[i], input(), nullptr, ec, ctx16, nullptr, &nxt, shared && i == 1));    // shared: B/2 rows in, B rows out
            }
            h = std::move(nxt);
            hv = h;
            CHK(zero_conv(n.zero_convs[i], h, (int)i));
        }
        Act m;
        CHK(block_fwd(n.middle, input(), nullptr, ec, ctx16, nullptr, &m));
        return zero_conv(n.mid_out, m, -1);
    }

    // controlnet_fwd for every ControlNet of the engine (residuals into hs / h_mid, or deferred), each inside the scope that
    // `per_net(c)` returns: the list that records it and the arena that serves it
    template <class PerNet>
    int controlnets_fwd(const Tensor& x4, const int64_t* t, const float* tf, const Tensor& ctx16, const float* scales, std::vector<Act>* hs,
                        Act* h_mid, bool only_mid, bool pairs, std::vector<Deferred>* defer, PerNet per_net) {
        for (size_t c = 0; c < cns.size(); ++c) {
            RecordScope scope = per_net(c);
            CHK(controlnet_fwd(cns[c], x4, t, tf, ctx16, scales ? scales + 13 * c : nullptr, hs, h_mid, only_mid, nullptr, 0, pairs, defer));
        }
        return FGDM_OK;
    }

    int apply_model(const float* x, const int64_t* t, const float* tf, const float* ctx, const float* pcond,
                    const float* scales, int B, int H, int W, int flags, float* eps_out) {
        if (!cap.on) return apply_model_walk(x, t, tf, ctx, pcond, scales, B, H, W, flags, eps_out);
        if (!finalized) return fail(FGDM_ERR_STATE, "weights not finalized");
        if (B <= 0 || H <= 0 || W <= 0) return fail(FGDM_ERR_ARG, "bad shape");
        CHK(capture_begin(B, H, W));
        const int rc = apply_model_walk(x, t, tf, ctx, pcond, scales, B, H, W, flags, eps_out);
        cap.capturing = false;
        return rc;
    }
    int apply_model_walk(const float* x, const int64_t* t, const float* tf, const float* ctx, const float* pcond,
                         const float* scales, int B, int H, int W, int flags, float* eps_out) {
        if (!finalized) return fail(FGDM_ERR_STATE, "weights not finalized");
        if (B <= 0 || H <= 0 || W <= 0) return fail(FGDM_ERR_ARG, "bad shape");
        Net& n = unet;
        const int HW = H * W;
        const int Cc = cfg.in_channels - 4;     // > 0: the first layer reads x | the c_concat cached by fgdm_set_concat
        if (Cc > 0) {
            if (!ccat.p) return fail(FGDM_ERR_STATE, "in_channels > 4 but no c_concat was registered (fgdm_set_concat)");
            if (!(ccat.B == B || (B % 2 == 0 && 2 * ccat.B == B)))
                return fail(FGDM_ERR_STATE, "the registered c_concat has " + std::to_string(ccat.B) + " rows: the batch must have as many, or twice as many");
            if (ccat.H != H || ccat.W != W) return fail(FGDM_ERR_STATE, "the registered c_concat has another latent size than x");
        }
        Act x4, ctx16;
        Buf emb;
        // FGDM_TWIN_STREAMS=1: between the fork and the join wait the second stream reads x4 / ctx16 / emb and writes the deferred
        // block outputs, and the main stream does not wait for it.  Whatever path leaves in between, the second stream is drained
        // BEFORE any of those blocks goes back to an arena (declared after them: destroyed before them, and before `deferred`).
        struct SecondStreamGuard {
            hipStream_t busy = nullptr;
            ~SecondStreamGuard() { if (busy) (void)hipStreamSynchronize(busy); }
        };
        CHK(talloc(&x4, B, H, W, Cc > 0 ? n.input[0][0].conv.cin_pad : 4));
        if (ctx) CHK(talloc(&ctx16, B, 1, ctx_tokens, cfg.context_dim));
        else if (ctx_B != B) return fail(FGDM_ERR_STATE, "ctx is NULL but no context of this batch size was registered (fgdm_set_context)");
        const bool pairs = (flags & FGDM_FLAG_CFG_PAIRS) && (B % 2 == 0) && n.input.size() > 1;      // (see below)
        if (Cc > 0) {      // only the rows the first layer reads: with CFG pairs the shared half, rows [0, B/2) of x and of the stored
                           // c_concat, whether that holds B/2 rows or B (the caller's word that rows b and b + B/2 are equal)
            const int rows = pairs ? B / 2 : B;
            if (pack_xcat(x, ccat.p, x4.p, rows, std::min(ccat.B, rows), Cc, HW, x4.C, s) != FGDM_OK) return fail(FGDM_ERR_HIP, "pack kernel");
        } else if (nchw_f32_to_nhwc_f16(x, x4.p, B, 4, HW, 4, s) != FGDM_OK) return fail(FGDM_ERR_HIP, "layout kernel");
        if (ctx && f32_to_f16(ctx, ctx16.p, ctx16.numel(), s) != FGDM_OK) return fail(FGDM_ERR_HIP, "convert kernel");
        CHK(embed(n, t, tf, B, &emb));
        EmbCtx ec{emb.as<float>(), n.emb_total};

        const bool use_adapter = n.has_adapter && !(flags & FGDM_FLAG_USE_ORIGINAL);
        // FGDM_FLAG_CFG_PAIRS: the batch is cat([x] * 2) of a classifier-free-guidance step (ddim.py:222-226): rows b and
        // b + B/2 have the same x, t (and pcond / hint) and differ only in the context.  Everything before the first
        // cross-attention -- conv_in, the first ResBlock, the first self-attention, the adapter -- is computed once on
        // B/2 rows and duplicated where the context enters.  Per-sample results are unchanged bit for bit.
        const int Bs = pairs ? B / 2 : B;              // rows of the shared prefix
        Tensor x4s = x4; x4s.B = Bs;
        Act fa[4];
        if (use_adapter) {
            if (pcond) {
                Act p4;
                CHK(talloc(&p4, Bs, H, W, 4));
                if (nchw_f32_to_nhwc_f16(pcond, p4.p, Bs, 4, HW, 4, s) != FGDM_OK) return fail(FGDM_ERR_HIP, "layout kernel");
                CHK(n.time_adapter ? time_adapter_fwd(n, p4, ec, fa) : adapter_fwd(n, p4, fa));
            } else {
                CHK(n.time_adapter ? time_adapter_fwd(n, x4s, ec, fa) : adapter_fwd(n, x4s, fa));
            }
        }
        // ---- the ControlNets are independent of the UNet's encoder + middle block (cldm.py:40,46).  Twin streams: they run next to it
        const bool with_cn = !cns.empty() && !(flags & FGDM_FLAG_NO_CONTROL);
        const bool twin = twin_streams && with_cn && s2 && !(flags & FGDM_FLAG_ONLY_MID_CONTROL);
        std::vector<Deferred> deferred;
        // ---- grouped twin launches: record the ControlNet walks, then the UNet encoder + middle block, and replay them together
        const bool paired = pair_launch && with_cn && !twin && !(flags & FGDM_FLAG_ONLY_MID_CONTROL);
        // ---- encoder (openaimodel.py:849-858); the adapter feature is added BEFORE the skip is recorded
        std::vector<Act> hs;      // every input block's output: the skip tensors, each also read (not consumed) by the next block
        Act hm;
        SecondStreamGuard second;
        auto encoder = [&]() -> int {
            LayerHints twins(*this, with_cn);                // encoder + middle block: the ControlNets' twins
            int k = 0;
            Act h0s;           // input block 0 on the shared rows (CFG pairs)
            for (size_t i = 0; i < n.input.size(); ++i) {
                Act nxt;
                if (pairs && i == 0) {
                    CHK(block_fwd(n.input[0], borrow(x4s), nullptr, ec, ctx16, nullptr, &h0s));
                    CHK(dup_rows(h0s, &nxt));                                        // the skip tensor hs[0] needs all B rows
                } else if (pairs && i == 1) {
                    CHK(block_fwd(n.input[1], std::move(h0s), nullptr, ec, ctx16, nullptr, &nxt, true));   // B/2 rows in, B rows out
                } else {
                    CHK(block_fwd(n.input[i], borrow(i == 0 ? x4 : hs.back()), nullptr, ec, ctx16, nullptr, &nxt));
                }
                if (use_adapter && (i + 1) % 3 == 0) {
                    // the adapter features cover Bs rows; with CFG pairs each is added to both halves
                    if (k >= 4 || fa[k].numel() * (size_t)(B / Bs) != nxt.numel()) return fail(FGDM_ERR_ARG, "adapter feature shape mismatch (latent size must be divisible by 8)");
                    for (int half = 0; half < B / Bs; ++half) {
                        half_t* dst = nxt.p + (size_t)half * fa[k].numel();
                        if (n.xad_valid) {   // h = h + fk + fa[adapter_idx] (openaimodel.py:1301-1305): fk first, like the reference's sum order
                            if (n.xad_sum[k].numel() != nxt.numel()) return fail(FGDM_ERR_ARG, "registered adapter conds do not match this batch / latent size");
                            const half_t* xs = n.xad_sum[k].p + (size_t)half * fa[k].numel();
                            if (add_f16(dst, xs, dst, fa[k].numel(), s) != FGDM_OK) return fail(FGDM_ERR_HIP, "add kernel");
                        }
                        if (add_f16(dst, fa[k].p, dst, fa[k].numel(), s) != FGDM_OK) return fail(FGDM_ERR_HIP, "add kernel");
                    }
                    fa[k].reset();
                    ++k;
                }
                hs.push_back(std::move(nxt));
            }
            return block_fwd(n.middle, borrow(hs.back()), nullptr, ec, ctx16, nullptr, &hm);
        };
        if (paired) {
            std::vector<RecWalk> walks(1 + cns.size());      // the UNet's, then one per ControlNet
            {
                const bool fat = knob_once(KNOB_PAIR_FAT_TILES) != 0;      // A/B knob
                LayerHints fused(*this, false, fat ? std::min<int>(group_max, 1 + (int)cns.size()) : 0);
                groupnorm_set_group(gn_group);
                CHK(controlnets_fwd(x4, t, tf, ctx16, scales, nullptr, nullptr, false, pairs, &deferred,         // an arena per walk: see cn_arena
                                    [&](size_t c) { return RecordScope(*this, &walks[1 + c], cn_arena[c].get()); }));
                RecordScope rec(*this, &walks[0], &arena);
                CHK(encoder());
            }
            // the UNet and ALL its ControlNets in one lockstep replay (FGDM_GROUP_MAX=2: pairwise, as in round 3)
            std::vector<RecWalk*> lists;
            for (RecWalk& w : walks) lists.push_back(&w);
            CHK(fgdm_replay(lists, group_max, s, prof, replay_stats));
        } else {
            if (twin) {      // the ControlNets start now, on the second stream, next to the UNet encoder
                if (hipEventRecord(ev_fork, s) != hipSuccess || hipStreamWaitEvent(s2, ev_fork, 0) != hipSuccess) return fail(FGDM_ERR_HIP, "stream fork");
                second.busy = s2;
                hipStream_t main_s = s;
                s = s2;
                const int rc = controlnets_fwd(x4, t, tf, ctx16, scales, nullptr, nullptr, false, pairs, &deferred,
                                               [&](size_t) { return RecordScope(*this, nullptr, cn_arena[0].get()); });
                s = main_s;
                if (rc != FGDM_OK) return rc;
                if (hipEventRecord(ev_join, s2) != hipSuccess) return fail(FGDM_ERR_HIP, "stream join");
            }
            CHK(encoder());
        }
        // ---- ControlNets: residuals accumulate in place into hs / hm (cldm.py:40,46,846)
        if (twin || paired) {
            if (twin && hipStreamWaitEvent(s, ev_join, 0) != hipSuccess) return fail(FGDM_ERR_HIP, "stream join");
            second.busy = nullptr;      // from here on the main stream is ordered behind the second
            for (const Deferred& d : deferred) CHK(zero_conv_into(*d.w, d.src, d.idx < 0 ? hm : hs[d.idx], d.scale));
            // the ControlNets' block outputs go back to their own arena: its next user is the next call's second stream, which
            // waits for that call's fork event, recorded behind these zero-convs
            deferred.clear();
        } else if (with_cn) {
            CHK(controlnets_fwd(x4, t, tf, ctx16, scales, &hs, &hm, (flags & FGDM_FLAG_ONLY_MID_CONTROL) != 0, pairs, nullptr,
                                [&](size_t) { return RecordScope(*this, nullptr, &arena); }));
        }
        // ---- decoder (openaimodel.py:868-870): virtual concat [h, skip]
        Act h = std::move(hm);
        for (size_t i = 0; i < n.output.size(); ++i) {
            Act skip = std::move(hs.back()), nxt;      // the skip goes back when the block is done
            hs.pop_back();
            CHK(block_fwd(n.output[i], std::move(h), &skip, ec, ctx16, nullptr, &nxt));
            h = std::move(nxt);
        }
        // ---- out: GN -> SiLU -> conv3x3 (openaimodel.py:724-728) straight to fp32 NCHW
        Act g;
        CHK(gnorm(n.out_gn, h, nullptr, 1e-5f, true, &g));
        h.reset();
        Epi e; e.out_kind = OUT_F32_NCHW; e.out = eps_out; e.ld_out = HW;
        return conv3(n.out_conv, g, nullptr, 1, false, e, nullptr);      // g, x4, ctx16 and emb go back behind it
    }

    // ------------------------------------------------------------------------------------ text encoder
    // CLIPTextModel.forward -> last_hidden_state (pre-LN transformer, causal attention, quick-GELU MLP)
    // clip_skip > 1: final_layer_norm(hidden_states[-clip_skip]) (controlnet/cldm/hack.py:40-45); hidden_states[-k] is the output
    // of layer L - k + 1 of L, so the last clip_skip - 1 layers are not run
    int clip_encode(const int64_t* ids, int B, int T, float* out, int clip_skip = 0) {
        if (!clip.on) return fail(FGDM_ERR_STATE, "engine was created without a text encoder (clip_layers = 0)");
        if (!comps[clip_comp].packed) return fail(FGDM_ERR_STATE, "weights not finalized");
        if (B <= 0 || T <= 0 || T > cfg.clip_max_len) return fail(FGDM_ERR_ARG, "bad shape (T must be <= clip_max_len)");
        if (clip_skip > cfg.clip_layers + 1) return fail(FGDM_ERR_ARG, "clip_skip exceeds the number of hidden states");
        const int n_run = cfg.clip_layers - (clip_skip > 1 ? clip_skip - 1 : 0);
        int li = 0;
        const int W = cfg.clip_width, rows = B * T;
        // the hidden states are an fp32 residual stream, as under the reference's autocast: fp32 embeddings, every branch
        // (attention / MLP output, a fp16 GEMM result) is promoted when added to it, LayerNorm reads fp32
        Act n, qkv, a, f;
        Buf hb, h2b;
        CHK(balloc(&hb, (size_t)rows * W * sizeof(float)));
        CHK(balloc(&h2b, (size_t)rows * W * sizeof(float)));
        float *const h = hb.as<float>(), *const h2 = h2b.as<float>();
        if (embed_tokens(ids, clip.tok, clip.pos, h, rows, T, W, cfg.clip_vocab, s) != FGDM_OK) return fail(FGDM_ERR_HIP, "embedding kernel");
        auto ln32 = [&](const NormW& nw, const float* src, Act* dst) -> int {
            CHK(talloc(dst, 1, 1, rows, W));
            return layernorm32_launch(src, rows, W, nw.g, nw.b, 1e-5f, dst->p, nullptr, s) == FGDM_OK ? FGDM_OK : fail(FGDM_ERR_HIP, "layernorm");
        };
        for (const ClipLayer& l : clip.layers) {
            if (li++ >= n_run) break;
            CHK(ln32(l.ln1, h, &n));
            CHK(linear(l.qkv, n, Epi{}, &qkv));
            n.reset();
            CHK(talloc(&a, 1, 1, rows, W));
            if (small_attention_launch(qkv.p, 3 * W, W, 2 * W, a.p, W, B, cfg.clip_heads, T, W / cfg.clip_heads, 1, s) != FGDM_OK)
                return fail(FGDM_ERR_HIP, "text attention kernel");
            qkv.reset();
            Act br;
            CHK(linear(l.o, a, Epi{}, &br));                 // branch output fp16, as autocast leaves it
            a.reset();
            if (add_f16_to_f32(h, br.p, h2, br.numel(), s) != FGDM_OK) return fail(FGDM_ERR_HIP, "add kernel");
            br.reset();
            CHK(ln32(l.ln2, h2, &n));
            { Epi e; e.act = ACT_QGELU; CHK(linear(l.fc1, n, e, &f)); }
            n.reset();
            CHK(linear(l.fc2, f, Epi{}, &br));
            f.reset();
            if (add_f16_to_f32(h2, br.p, h, br.numel(), s) != FGDM_OK) return fail(FGDM_ERR_HIP, "add kernel");
        }
        // final_layer_norm: fp32 in, fp32 out -- straight into the caller's buffer
        if (layernorm32_launch(h, rows, W, clip.final_ln.g, clip.final_ln.b, 1e-5f, nullptr, out, s) != FGDM_OK) return fail(FGDM_ERR_HIP, "layernorm");
        return FGDM_OK;
    }

    // ------------------------------------------------------------------------------------ first-stage decoder
    // AttnBlock.forward (model.py:176-203): ONE head over all C channels.  d = C = 512 does not fit the flash kernel's
    // register budget, so per image: S = C^-1/2 Q K^T (fp32, GEMM with K as the "weight"), row softmax, O = P V
    // (GEMM with V^T, written transposed by the v projection's epilogue, as the weight).
    int vattn_fwd(const VAttn& at, const Tensor& x, Act* out) {
        const int B = x.B, T = x.H * x.W, C = x.C;
        if (T & 63) return fail(FGDM_ERR_ARG, "first-stage attention: H*W must be a multiple of 64");
        Act g, q, k, vt, a, P;
        Buf S;
        CHK(gnorm(at.norm, x, nullptr, 1e-6f, false, &g));
        CHK(linear(at.q, g, Epi{}, &q));
        CHK(talloc(&k, 1, 1, B * T + 128, C));        // + 128 rows: the GEMM reads whole 128-row weight tiles
        CHK(talloc(&vt, B, 1, C, T));
        CHK(talloc(&a, B, x.H, x.W, C));
        CHK(talloc(&P, 1, 1, T, T));
        CHK(balloc(&S, (size_t)T * T * sizeof(float)));
        HIP_TRY(hipMemsetAsync(k.p + (size_t)B * T * C, 0, (size_t)128 * C * sizeof(half_t), s));
        { Epi e; e.out = k.p; e.ld_out = C; e.rps = T; CHK(linear(at.k, g, e, nullptr)); }
        { Epi e; e.out_kind = OUT_F16_T; e.out = vt.p; e.ld_out = T; e.rps = T; CHK(linear(at.v, g, e, nullptr)); }
        g.reset();
        bool softmax_failed = false;
        const int rc = vattn_core(q.p, k.p, vt.p, a.p, S.as<float>(), P.p, B, T, C, s, &softmax_failed,
            [&](const half_t* Wt, int N, int K, const half_t* A, int M, int out_kind, void* o, int ld_out, float scale) {
                GemmW w; w.w = const_cast<half_t*>(Wt); w.N = N; w.K = K; w.k_real = K;
                Tensor xa; xa.p = const_cast<half_t*>(A); xa.B = 1; xa.H = 1; xa.W = M; xa.C = K;
                Epi e; e.out_kind = out_kind; e.out = o; e.ld_out = ld_out; e.rps = M; e.scale = scale;
                return gemm(w, IG_LINEAR, xa, nullptr, 1, M, e, nullptr);
            });
        if (rc != FGDM_OK) return softmax_failed ? fail(rc, "softmax kernel") : rc;
        S.reset(); P.reset(); q.reset(); k.reset(); vt.reset();
        Epi e; e.resid = x.p; e.ld_res = C;
        return linear(at.o, a, e, out);
    }
    // LatentDiffusion.decode_first_stage (ddpm.py:839,889) -> AutoencoderKL.decode (autoencoder.py:330-333) ->
    // Decoder.forward (model.py:532-560).  z fp32 NCHW [B,4,H,W] -> image fp32 NCHW [B,out_ch,f*H,f*W]
    int vae_decode(const float* z, int B, int H, int W, float scale, float* out) {
        if (!vae.on) return fail(FGDM_ERR_STATE, "engine was created without a first-stage decoder (vae_ch = 0)");
        if (!comps[vae_comp].packed) return fail(FGDM_ERR_STATE, "weights not finalized");
        if (B <= 0 || H <= 0 || W <= 0) return fail(FGDM_ERR_ARG, "bad shape");
        const Vae& v = vae;
        const int f = v.factor, HW = H * W;
        const EmbCtx no_emb{nullptr, 0};
        const size_t out_per_img = (size_t)cfg.vae_out_ch * H * f * W * f;
        // images per pass: ~8 live full-resolution tensors of `ch` channels must fit comfortably in one slab
        const size_t big = (size_t)H * f * W * f * cfg.vae_ch * sizeof(half_t) * 8;
        const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)B, ((size_t)3 << 30) / std::max<size_t>(big, 1)));
        for (int b0 = 0; b0 < B; b0 += chunk) {
            const int nb = std::min(chunk, B - b0);
            Act z4, h, t, g;
            CHK(talloc(&z4, nb, H, W, 4));
            if (vae_prequant(z + (size_t)b0 * 4 * HW, v.pq, scale, z4.p, nb, HW, s) != FGDM_OK) return fail(FGDM_ERR_HIP, "prequant kernel");
            CHK(conv3(v.conv_in, z4, nullptr, 1, false, Epi{}, &h));
            z4.reset();
            CHK(res_fwd(v.mid1, h, nullptr, no_emb, &t)); h = std::move(t);
            CHK(vattn_fwd(v.attn, h, &t)); h = std::move(t);
            CHK(res_fwd(v.mid2, h, nullptr, no_emb, &t)); h = std::move(t);
            for (const VLevel& lv : v.levels) {
                for (const Layer& r : lv.blocks) { CHK(res_fwd(r, h, nullptr, no_emb, &t)); h = std::move(t); }
                if (lv.up) { CHK(conv3(lv.upconv, h, nullptr, 1, true, Epi{}, &t)); h = std::move(t); }
            }
            CHK(gnorm(v.norm_out, h, nullptr, 1e-6f, true, &g));
            h.reset();
            { Epi e; e.out_kind = OUT_F32_NCHW; e.out = out + (size_t)b0 * out_per_img; e.ld_out = g.H * g.W;
              CHK(conv3(v.conv_out, g, nullptr, 1, false, e, nullptr)); }
        }
        return FGDM_OK;
    }

    // LatentDiffusion.encode_first_stage (ddpm.py:952-996, plain branch) -> AutoencoderKL.encode (autoencoder.py:324-328) ->
    // Encoder.forward (model.py:436-460) + quant_conv.  image fp32 NCHW [B,3,H,W] -> moments fp32 NCHW [B,2*z_channels,H/f,W/f]
    int vae_encode(const float* image, int B, int H, int W, float* moments) {
        if (!vae.on || !vae.enc.on) return fail(FGDM_ERR_STATE, "engine was created without a first-stage encoder (vae_encoder = 0)");
        if (!comps[vae_comp].packed) return fail(FGDM_ERR_STATE, "weights not finalized");
        const VEnc& en = vae.enc;
        const int f = vae.factor;
        const EmbCtx no_emb{nullptr, 0};
        if (B <= 0 || H <= 0 || W <= 0 || H % f || W % f || (((H / f) * (W / f)) & 63))
            return fail(FGDM_ERR_ARG, "first-stage encoder: H and W must be multiples of " + std::to_string(f) + " and (H/" + std::to_string(f) +
                                      ")*(W/" + std::to_string(f) + ") a multiple of 64 (smallest image 64 x 64)");
        const int hw = (H / f) * (W / f), zc2 = 2 * cfg.vae_z_channels;
        // images per pass: ~8 live full-resolution tensors of `ch` channels must fit comfortably in one slab (as vae_decode)
        const size_t big = (size_t)H * W * cfg.vae_ch * sizeof(half_t) * 8;
        const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)B, ((size_t)3 << 30) / std::max<size_t>(big, 1)));
        for (int b0 = 0; b0 < B; b0 += chunk) {
            const int nb = std::min(chunk, B - b0);
            Act x4, h, t, g;
            Buf h32;                                                     // conv_out, fp32 [pixel][2 z_channels]
            CHK(talloc(&x4, nb, H, W, en.conv_in.cin_pad));              // 3 -> 4 channels
            if (nchw_f32_to_nhwc_f16(image + (size_t)b0 * 3 * H * W, x4.p, nb, 3, H * W, x4.C, s) != FGDM_OK) return fail(FGDM_ERR_HIP, "layout kernel");
            CHK(conv3(en.conv_in, x4, nullptr, 1, false, Epi{}, &h));
            x4.reset();
            for (const VDown& lv : en.levels) {
                for (const Layer& r : lv.blocks) { CHK(res_fwd(r, h, nullptr, no_emb, &t)); h = std::move(t); }
                if (lv.down) { CHK(conv3(lv.downconv, h, nullptr, FGDM_STRIDE2_PAD_BR, false, Epi{}, &t)); h = std::move(t); }
            }
            CHK(res_fwd(en.mid1, h, nullptr, no_emb, &t)); h = std::move(t);
            CHK(vattn_fwd(en.attn, h, &t)); h = std::move(t);
            CHK(res_fwd(en.mid2, h, nullptr, no_emb, &t)); h = std::move(t);
            CHK(gnorm(en.norm_out, h, nullptr, 1e-6f, true, &g));
            h.reset();
            CHK(balloc(&h32, (size_t)nb * hw * zc2 * sizeof(float)));
            { Epi e; e.out_kind = OUT_F32; e.out = h32.p; e.ld_out = zc2; CHK(conv3(en.conv_out, g, nullptr, 1, false, e, nullptr)); }
            g.reset();
            if (vae_moments(h32.as<float>(), en.qc, moments + (size_t)b0 * zc2 * hw, nb, hw, s) != FGDM_OK) return fail(FGDM_ERR_HIP, "moments kernel");
        }
        return FGDM_OK;
    }

    // input_hint_block (cldm.py:655-671): 8 conv3x3, SiLU between, stride 2 at convs 2/4/6; result cached
    int set_hint(int cn, const float* hint, int B, int Hh, int Wh) {
        if (!finalized) return fail(FGDM_ERR_STATE, "weights not finalized");
        if (cn < 0 || cn >= (int)cns.size()) return fail(FGDM_ERR_ARG, "no such ControlNet");
        if ((Hh & 7) || (Wh & 7) || B <= 0) return fail(FGDM_ERR_ARG, "hint size must be a multiple of 8");
        Net& n = cns[cn];
        const int mc = cfg.model_channels, Hl = Hh / 8, Wl = Wh / 8;
        if (n.guided.p && (n.guided.B != B || n.guided.H != Hl || n.guided.W != Wl)) { (void)hipFree(n.guided.p); n.guided.p = nullptr; }
        if (!n.guided.p) {
            n.guided.B = B; n.guided.H = Hl; n.guided.W = Wl; n.guided.C = mc;
            if (hipMalloc(&n.guided.p, n.guided.numel() * sizeof(half_t)) != hipSuccess) return fail(FGDM_ERR_NOMEM, "hipMalloc (hint cache)");
        }
        const int hc = n.hint_convs[0].cin_pad;   // 3 -> 4
        const int chunk = std::max(1, std::min(B, (int)(((size_t)512 << 20) / ((size_t)Hh * Wh * 192 * 2 + 1))));
        for (int b0 = 0; b0 < B; b0 += chunk) {
            const int nb = std::min(chunk, B - b0);
            Act cur;
            CHK(talloc(&cur, nb, Hh, Wh, hc));
            if (nchw_f32_to_nhwc_f16(hint + (size_t)b0 * cfg.hint_channels * Hh * Wh, cur.p, nb, cfg.hint_channels, Hh * Wh, hc, s) != FGDM_OK)
                return fail(FGDM_ERR_HIP, "layout kernel");
            for (int k = 0; k < 8; ++k) {
                const int stride = (k == 2 || k == 4 || k == 6) ? 2 : 1;
                Epi e;
                e.act = k < 7 ? ACT_SILU : ACT_NONE;
                Act nxt;
                if (k == 7) { e.out = n.guided.p + (size_t)b0 * Hl * Wl * mc; e.ld_out = mc; }
                CHK(conv3(n.hint_convs[k], cur, nullptr, stride, false, e, k == 7 ? nullptr : &nxt));
                cur = std::move(nxt);
            }
        }
        return FGDM_OK;
    }

    // c_concat of DiffusionWrapper's 'hybrid' mode (ddpm.py:1838-1841): the same tensor in every step of a sampling, so it is
    // converted once -- fp32 NCHW [B, Cc, H, W] -> fp16 NHWC, rounded as x is -- and apply_model packs it behind x (k_pack_xcat)
    void drop_concat() { if (ccat.p) (void)hipFree(ccat.p); ccat = Tensor{}; }
    int set_concat(const float* cc, int B, int Cc, int H, int W) {
        if (cfg.in_channels == 4) return fail(FGDM_ERR_ARG, "fgdm_set_concat: this engine's UNet takes x alone (in_channels = 4)");
        if (!cc) { drop_concat(); return FGDM_OK; }
        // a refused tensor leaves NOTHING stored: a caller who ignores the return code gets FGDM_ERR_STATE from apply_model, not the
        // previous image
        if (Cc != cfg.in_channels - 4) {
            drop_concat();
            return fail(FGDM_ERR_ARG, "fgdm_set_concat: c_concat must have in_channels - 4 = " + std::to_string(cfg.in_channels - 4) + " channels");
        }
        if (B <= 0 || H <= 0 || W <= 0) { drop_concat(); return fail(FGDM_ERR_ARG, "bad shape"); }
        if (ccat.p && (ccat.B != B || ccat.H != H || ccat.W != W)) drop_concat();
        if (!ccat.p) {
            ccat.B = B; ccat.H = H; ccat.W = W; ccat.C = Cc;
            if (hipMalloc(&ccat.p, ccat.numel() * sizeof(half_t)) != hipSuccess) { ccat = Tensor{}; return fail(FGDM_ERR_NOMEM, "hipMalloc (c_concat cache)"); }
        }
        if (nchw_f32_to_nhwc_f16(cc, ccat.p, B, Cc, H * W, Cc, s) != FGDM_OK) return fail(FGDM_ERR_HIP, "layout kernel");
        return FGDM_OK;
    }
};

// ================================================================================================ C ABI
// (the op-level test entries are in ops_abi.hip, the micro-benchmark entries in bench_abi.hip)
static std::string g_create_err;   // why the last fgdm_create / parameter-table query failed (there is no engine to ask): fgdm_last_error(NULL)

static int make_desc(const fgdm_config* cfg, fgdm_engine** out) {
    fgdm_engine* e = new fgdm_engine();
    e->cfg = *cfg;
    const int rc = e->build();
    if (rc != FGDM_OK) { g_create_err = "unsupported configuration: " + e->err; delete e; return rc; }
    *out = e;
    return FGDM_OK;
}

// One C-ABI call that uses the activation workspace, on the caller's stream and the main arena.  Whatever it returns, the handles
// it held have given their blocks back by then (arena.h).
template <typename F> static int stream_call(fgdm_engine* e, void* stream, F f) {
    e->s = as_stream(stream);
    e->ar = &e->arena;
    return f();
}

// ------------------------------------------------------------------------------------------------ device sampler loops: the driver
// The caller's struct in the library's layout.  It may be any version this library knows: at least the first one, at most this
// one; the fields its version did not have yet read as zero (absent).  false: a larger size holds fields this library cannot honour.
static bool read_params(const void* caller, int64_t size_v1, void* known, size_t size_lib) {
    int64_t size;
    memcpy(&size, caller, sizeof(size));      // struct_size leads every parameter struct
    if (size < size_v1 || size > (int64_t)size_lib) return false;
    memset(known, 0, size_lib);
    memcpy(known, caller, (size_t)size);
    return true;
}

// The network's time argument of every evaluation: host entry k, Bm times, at dev[k * Bm].
template <typename T> static int upload_repeated(const T* host, int count, int Bm, T* dev, hipStream_t s) {
    std::vector<T> th((size_t)count * Bm);
    for (int k = 0; k < count; ++k) for (int b = 0; b < Bm; ++b) th[(size_t)k * Bm + b] = host[k];
    HIP_TRY(hipMemcpyAsync(dev, th.data(), th.size() * sizeof(T), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));   // th is a local: the copy must finish before it goes out of scope
    return FGDM_OK;
}

// CFG of a loop: on when uncond is given and the scale is not 1, and then the loop owns FGDM_FLAG_CFG_PAIRS
static bool loop_cfg_on(const float* uncond, float cfg_scale) { return uncond && cfg_scale != 1.0f; }
static int loop_flags(int flags, bool cfg_on) { return cfg_on ? flags | FGDM_FLAG_CFG_PAIRS : flags & ~FGDM_FLAG_CFG_PAIRS; }

// The driver of the six device loops (inside the entry's stream_call).  It owns what every loop holds while it runs -- the
// network's input x2 (Bm rows: cat([x] * 2), or x with CFG off), its output eps, the loop-invariant context cat([uncond, cond])
// (ddim.py:226), registered (projected) once so that every evaluation passes ctx = NULL, the history planes an entry asks for and
// the device time table (int64 timesteps or fractional times, whichever the entry has) -- and does every allocation, copy and
// network evaluation of a loop.  An entry keeps its coefficients, its history rotation and its step kernel.
struct Loop {
    fgdm_engine* e;
    hipStream_t s;
    float* x;                       // the caller's state
    const float* control_scales;
    int B, H, W, K, flags;          // K evaluations' times; the flags as the entry resolved them
    bool cfg_on;
    const int32_t* log_steps;
    int n_log;
    Buf x2_buf, eps_buf, c2_buf, hist_buf, t_buf;      // ... which go back to the arena with the Loop
    float *x2 = nullptr, *eps = nullptr, *c2 = nullptr, *hist = nullptr;
    int64_t* t_int = nullptr;
    float* t_float = nullptr;
    int Bm = 0, logged = 0;
    size_t n = 0;

    // P: a public parameter struct, or a Walk
    template <typename P> Loop(fgdm_engine* e_, hipStream_t s_, const P& p, int K_, bool cfg_on_, int flags_, const int32_t* log_steps_ = nullptr, int n_log_ = 0)
        : e(e_), s(s_), x(p.x), control_scales(p.control_scales), B(p.B), H(p.H), W(p.W), K(K_), flags(flags_), cfg_on(cfg_on_),
          log_steps(log_steps_), n_log(n_log_) {}

    int begin(const float* cond, const float* uncond, const int64_t* times_int, const float* times_float, int hist_planes) {
        Bm = cfg_on ? 2 * B : B;
        n = (size_t)B * 4 * H * W;
        const size_t nctx = (size_t)B * e->ctx_tokens * e->cfg.context_dim;
        CHK(e->balloc(&x2_buf, Bm * 4 * (size_t)H * W * sizeof(float)));
        CHK(e->balloc(&eps_buf, Bm * 4 * (size_t)H * W * sizeof(float)));
        CHK(e->balloc(&c2_buf, Bm * (size_t)e->ctx_tokens * e->cfg.context_dim * sizeof(float)));
        x2 = x2_buf.as<float>(); eps = eps_buf.as<float>(); c2 = c2_buf.as<float>();
        if (cfg_on) {
            HIP_TRY(hipMemcpyAsync(c2, uncond, nctx * sizeof(float), hipMemcpyDeviceToDevice, s));
            HIP_TRY(hipMemcpyAsync(c2 + nctx, cond, nctx * sizeof(float), hipMemcpyDeviceToDevice, s));
        } else {
            HIP_TRY(hipMemcpyAsync(c2, cond, nctx * sizeof(float), hipMemcpyDeviceToDevice, s));
        }
        CHK(e->set_context(c2, Bm));
        if (hist_planes) CHK(e->balloc(&hist_buf, hist_planes * n * sizeof(float)));
        CHK(e->balloc(&t_buf, (size_t)K * Bm * (times_int ? sizeof(int64_t) : sizeof(float))));
        hist = hist_buf.as<float>();
        if (times_int) return upload_repeated(times_int, K, Bm, t_int = t_buf.as<int64_t>(), s);
        return upload_repeated(times_float, K, Bm, t_float = t_buf.as<float>(), s);
    }
    float* plane(int j) const { return hist + (size_t)j * n; }
    // x into the network's input, once, for the loops whose first launch is not a blend
    int seed() {
        HIP_TRY(hipMemcpyAsync(x2, x, n * sizeof(float), hipMemcpyDeviceToDevice, s));
        if (cfg_on) HIP_TRY(hipMemcpyAsync(x2 + n, x, n * sizeof(float), hipMemcpyDeviceToDevice, s));
        return FGDM_OK;
    }
    // the network on x2 at time table entry k
    int eval(int k) {
        return e->apply_model(x2, t_int ? t_int + (size_t)k * Bm : nullptr, t_float ? t_float + (size_t)k * Bm : nullptr, nullptr, nullptr,
                              control_scales, Bm, H, W, flags, eps);
    }
    void feed(StepIO& io) const { io.xin_a = x2; io.xin_b = cfg_on ? x2 + n : nullptr; }
    // the I/O of step i of K behind its evaluation: the input halves only when another evaluation follows
    StepIO step_io(int i, float cfg) const {
        StepIO io{};
        io.x = x; io.n = n; io.ec = cfg_on ? eps + n : eps; io.eu = cfg_on ? eps : nullptr; io.cfg = cfg; io.x_out = x;
        if (i + 1 < K) feed(io);
        return io;
    }
    // step i's slot in the log tensors, or -1: not logged
    int log_slot(int i) { return logged < n_log && log_steps[logged] == i ? logged++ : -1; }
    float* log_plane(float* out, int slot) const { return out && slot >= 0 ? out + (size_t)slot * n : nullptr; }
};

// What the six entries do in front of their loop, in this order: NULL engine or struct; the struct's size; the entry's own checks
// (`check`: nullptr / empty = consistent); hybrid networks; unfinalized weights; then `body(e, known, stream)` in a stream_call.
static std::string why_text(const char* why) { return why ? why : ""; }
static std::string why_text(const std::string& why) { return why; }
template <typename P, typename Check, typename Body>
static int loop_entry(fgdm_engine* e, const P* caller, void* stream, int64_t size_v1, const char* entry, const char* struct_name,
                      bool refuse_hybrid, Check check, Body body) {
    if (!e || !caller) return FGDM_ERR_ARG;
    const std::string name = entry;
    P known;
    if (!read_params(caller, size_v1, &known, sizeof(known)))
        return e->fail(FGDM_ERR_ARG, name + ": struct_size is not the sizeof(" + struct_name + ") of a known header version");
    const std::string why = why_text(check(known));
    if (!why.empty()) return e->fail(FGDM_ERR_ARG, name + ": " + why);
    if (refuse_hybrid && e->cfg.in_channels > 4) return e->fail(FGDM_ERR_ARG, name + ": in_channels > 4 (hybrid c_concat) is not taken by the device loops");
    if (!e->finalized) return e->fail(FGDM_ERR_STATE, "weights not finalized");
    return stream_call(e, stream, [&] { return body(e, known, as_stream(stream)); });
}

extern "C" {

int fgdm_create(const fgdm_config* cfg, int device, fgdm_engine** out) {
    if (!cfg || !out) return FGDM_ERR_ARG;
    fgdm_engine* e = nullptr;
    int rc = make_desc(cfg, &e);
    if (rc != FGDM_OK) return rc;      // make_desc left the reason in g_create_err
    e->device = device;
    e->ln_fold = knob_on(KNOB_LN_FOLD);
    rc = e->ensure_device();
    if (rc != FGDM_OK) {
        g_create_err = e->err + " [" + hipGetErrorString(hipGetLastError()) + "]";
        delete e;
        return rc;
    }
    e->twin_streams = knob_on(KNOB_TWIN_STREAMS);
    e->pair_launch = knob_on(KNOB_PAIR_LAUNCH);
    e->group_max = std::max(2, std::min(FGDM_MAX_GROUP, knob_int(KNOB_GROUP_MAX)));
    e->gn_group = knob_on(KNOB_GN_GROUP);
    if (e->twin_streams && !e->cns.empty()) {
        if (hipStreamCreateWithFlags(&e->s2, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&e->ev_join, hipEventDisableTiming) != hipSuccess) {
            g_create_err = "second stream could not be created";
            delete e;
            return FGDM_ERR_HIP;
        }
    }
    // one workspace arena per ControlNet, sized like the main one (the configured slab size applies to all of them)
    for (size_t c = 0; c < e->cns.size(); ++c) {
        e->cn_arena.emplace_back(new Arena());
        if (e->cfg.workspace_bytes > 0) e->cn_arena.back()->slab_bytes = (size_t)e->cfg.workspace_bytes;
    }
    *out = e;
    return FGDM_OK;
}

void fgdm_destroy(fgdm_engine* e) {
    if (!e) return;
    for (hipEvent_t ev : e->prof.pool) (void)hipEventDestroy(ev);
    for (auto& c : e->comps) for (void* p : c.allocs) (void)hipFree(p);
    e->drop_snapshot();
    if (e->zero) (void)hipFree(e->zero);
    for (auto& n : e->cns) if (n.guided.p) (void)hipFree(n.guided.p);
    e->drop_concat();
    e->drop_context();
    e->drop_adapter_conds();
    e->capture_free();
    if (knob_text(KNOB_PAIR_DEBUG) && e->replay_stats.replayed)
        fprintf(stderr, "[fgdm] grouped twin launches: %ld of %ld replayed launches were fused (%ld problems)\n", e->replay_stats.fused, e->replay_stats.replayed, e->replay_stats.problems);
    if (e->s2) { (void)hipStreamSynchronize(e->s2); (void)hipStreamDestroy(e->s2); }
    if (e->ev_fork) (void)hipEventDestroy(e->ev_fork);
    if (e->ev_join) (void)hipEventDestroy(e->ev_join);
    delete e;
}

const char* fgdm_last_error(const fgdm_engine* e) { return e ? e->err.c_str() : g_create_err.c_str(); }

static fgdm_engine* g_desc = nullptr;
static fgdm_config g_desc_cfg;
static fgdm_engine* desc_for(const fgdm_config* cfg) {
    if (g_desc && memcmp(&g_desc_cfg, cfg, sizeof(*cfg)) == 0) return g_desc;
    if (g_desc) { delete g_desc; g_desc = nullptr; }
    if (make_desc(cfg, &g_desc) != FGDM_OK) return nullptr;
    g_desc_cfg = *cfg;
    return g_desc;
}
int fgdm_param_count(const fgdm_config* cfg) {
    if (!cfg) return FGDM_ERR_ARG;
    fgdm_engine* d = desc_for(cfg);
    return d ? (int)d->order.size() : FGDM_ERR_ARG;
}
int fgdm_param_info(const fgdm_config* cfg, int index, char* name, int name_cap, int64_t* shape, int* ndim) {
    if (!cfg || !name || !shape || !ndim) return FGDM_ERR_ARG;
    fgdm_engine* d = desc_for(cfg);
    if (!d || index < 0 || index >= (int)d->order.size()) return FGDM_ERR_ARG;
    const std::string& n = d->order[index];
    if ((int)n.size() + 1 > name_cap) return FGDM_ERR_ARG;
    memcpy(name, n.c_str(), n.size() + 1);
    const auto& sh = d->params[n].shape;
    *ndim = (int)sh.size();
    for (size_t i = 0; i < sh.size(); ++i) shape[i] = sh[i];
    return FGDM_OK;
}

int fgdm_load_tensor(fgdm_engine* e, const char* key, const void* data, int dtype, const int64_t* shape, int ndim) {
    if (!e || !key || !data || !shape) return FGDM_ERR_ARG;
    auto it = e->params.find(key);
    if (it == e->params.end()) return e->fail(FGDM_ERR_ARG, std::string("unknown parameter key: ") + key);
    ParamSlot& ps = it->second;
    if ((int)ps.shape.size() != ndim) return e->fail(FGDM_ERR_ARG, std::string("rank mismatch for ") + key);
    for (int i = 0; i < ndim; ++i)
        if (ps.shape[i] != shape[i]) return e->fail(FGDM_ERR_ARG, std::string("shape mismatch for ") + key);
    const size_t n = ps.numel();
    ps.host.resize(n);
    if (dtype == FGDM_DTYPE_F32) {
        if (hipMemcpy(ps.host.data(), data, n * sizeof(float), hipMemcpyDefault) != hipSuccess) return e->fail(FGDM_ERR_HIP, "hipMemcpy failed");
    } else if (dtype == FGDM_DTYPE_F16) {
        std::vector<half_t> tmp(n);
        if (hipMemcpy(tmp.data(), data, n * sizeof(half_t), hipMemcpyDefault) != hipSuccess) return e->fail(FGDM_ERR_HIP, "hipMemcpy failed");
        for (size_t i = 0; i < n; ++i) ps.host[i] = (float)tmp[i];
    } else {
        return e->fail(FGDM_ERR_ARG, "unsupported dtype");
    }
    ps.loaded = true;
    e->comps[ps.comp].dirty = true;
    e->finalized = false;
    return FGDM_OK;
}

int fgdm_finalize_weights(fgdm_engine* e) {
    if (!e) return FGDM_ERR_ARG;
    int rc = e->ensure_device();
    if (rc != FGDM_OK) return rc;
    e->drop_derived();          // everything derived from the previous weights is stale
    e->upd_open = false;
    e->upd.clear();
    // only components whose tensors changed since the last call are packed again (their previous HBM copy is freed
    // first): loading the base checkpoint and then a ControlNet checkpoint does not re-pack or leak the UNet
    for (int c = 0; c < (int)e->comps.size(); ++c) { rc = e->repack(c); if (rc != FGDM_OK) return rc; }
    e->finalized = true;
    return FGDM_OK;
}

int fgdm_weights_begin_update(fgdm_engine* e) {
    if (!e) return FGDM_ERR_ARG;
    if (!e->finalized) return e->fail(FGDM_ERR_STATE, "weights not finalized: an update changes a packed engine (load with fgdm_load_tensor)");
    e->upd.clear();
    e->upd_open = true;
    return FGDM_OK;
}
int fgdm_weights_update_tensor(fgdm_engine* e, const char* key, const float* device_fp32, const int64_t* shape, int ndim) {
    if (!e || !key || !device_fp32 || !shape) return FGDM_ERR_ARG;
    return e->weights_update_tensor(key, device_fp32, shape, ndim);
}
int fgdm_weights_commit_update(fgdm_engine* e, void* stream) {
    if (!e) return FGDM_ERR_ARG;
    return e->weights_commit(as_stream(stream));
}
int fgdm_weights_snapshot(fgdm_engine* e, const char* const* keys, int n) {
    if (!e || n < 0 || (n && !keys)) return FGDM_ERR_ARG;
    return e->weights_snapshot(keys, n);
}
int fgdm_weights_restore(fgdm_engine* e, void* stream) {
    if (!e) return FGDM_ERR_ARG;
    return e->weights_restore(as_stream(stream));
}
int64_t fgdm_weights_snapshot_bytes(const fgdm_engine* e) { return e ? (int64_t)e->snapshot_bytes() : FGDM_ERR_ARG; }
int fgdm_weights_update_plan(const fgdm_config* cfg, const char* const* keys, int n, char* out, int out_cap) {
    if (!cfg || n < 0 || (n && !keys) || out_cap < 0 || (out_cap && !out)) return FGDM_ERR_ARG;
    fgdm_engine* d = desc_for(cfg);
    if (!d) return FGDM_ERR_ARG;
    std::unordered_map<std::string, int> want;
    for (int i = 0; i < n; ++i) {
        if (!keys[i] || !d->params.count(keys[i])) { g_create_err = std::string("unknown parameter key: ") + (keys[i] ? keys[i] : "(null)"); return FGDM_ERR_ARG; }
        want[keys[i]] = 1;
    }
    std::string text;
    for (const auto& unit : d->plan_units(knob_on(KNOB_LN_FOLD), [&](const std::string& k) { return want.count(k) != 0; })) {
        for (size_t i = 0; i < unit.size(); ++i) text += (i ? " " : "") + unit[i];
        text += "\n";
    }
    if ((int)text.size() + 1 <= out_cap) memcpy(out, text.c_str(), text.size() + 1);
    return (int)text.size() + 1;
}

int fgdm_profile_begin(fgdm_engine* e, int stride) {
    if (!e) return FGDM_ERR_ARG;
    e->prof.on = true;
    e->prof.stride = stride > 0 ? stride : 1;
    e->prof.counter = 0;
    e->prof.used = 0;
    e->prof.recs.clear();
    for (int c = 0; c < PC_COUNT; ++c) { e->prof.work[c] = 0; e->prof.bytes[c] = 0; }
    return FGDM_OK;
}
// out[class][4] = {device milliseconds, launches, algorithmic work (flops for classes 0/1, bytes for 2/3), algorithmic bytes};
// classes: 0 implicit-GEMM (conv / linear), 1 attention, 2 GroupNorm + LayerNorm, 3 im2col.  Synchronises the device.
int fgdm_profile_end(fgdm_engine* e, double* out) {
    if (!e || !out) return FGDM_ERR_ARG;
    e->prof.on = false;
    if (hipDeviceSynchronize() != hipSuccess) return e->fail(FGDM_ERR_HIP, "hipDeviceSynchronize failed");
    for (int c = 0; c < PC_COUNT * 4; ++c) out[c] = 0;
    for (auto& r : e->prof.recs) {
        if (!r.e1) continue;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, e->prof.pool[r.e0], e->prof.pool[r.e1]) != hipSuccess) continue;
        out[r.cls * 4 + 0] += ms;
        out[r.cls * 4 + 1] += 1;
    }
    for (int c = 0; c < PC_COUNT; ++c) { out[c * 4 + 2] = e->prof.work[c]; out[c * 4 + 3] = e->prof.bytes[c]; }
    // optional per-shape dump: FGDM_PROF_DUMP=<path>  ->  "tag <tab> launches <tab> total_ms <tab> work"
    if (const char* path = knob_text(KNOB_PROF_DUMP)) {
        std::map<std::string, std::array<double, 3>> agg;
        for (auto& r : e->prof.recs) {
            if (!r.e1) continue;
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, e->prof.pool[r.e0], e->prof.pool[r.e1]) != hipSuccess) continue;
            auto& a = agg[r.tag];
            a[0] += 1; a[1] += ms; a[2] += r.w;
        }
        if (FILE* f = fopen(path, "w")) {
            for (auto& kv : agg) fprintf(f, "%s\t%.0f\t%.4f\t%.6g\n", kv.first.c_str(), kv.second[0], kv.second[1], kv.second[2]);
            fclose(f);
        }
    }
    return FGDM_OK;
}
int fgdm_workspace_stats(fgdm_engine* e, int64_t* peak_bytes, int64_t* reserved_bytes) {
    if (!e || !peak_bytes || !reserved_bytes) return FGDM_ERR_ARG;
    // all arenas: the main one and the ControlNets' (with grouped launches every ControlNet activation lives in those)
    size_t pk = e->arena.peak, r = e->arena.reserved();
    for (auto& a : e->cn_arena) { pk += a->peak; r += a->reserved(); }
    *peak_bytes = (int64_t)pk;
    *reserved_bytes = (int64_t)r;
    return FGDM_OK;
}

int fgdm_launch_stats(fgdm_engine* e, int64_t* replayed_launches, int64_t* fused_launches, int64_t* fused_problems) {
    if (!e || !replayed_launches || !fused_launches || !fused_problems) return FGDM_ERR_ARG;
    *replayed_launches = (int64_t)e->replay_stats.replayed;
    *fused_launches = (int64_t)e->replay_stats.fused;
    *fused_problems = (int64_t)e->replay_stats.problems;
    return FGDM_OK;
}

int fgdm_set_hint(fgdm_engine* e, int cn, const float* hint, int B, int Hh, int Wh, void* stream) {
    if (!e || !hint) return FGDM_ERR_ARG;
    return stream_call(e, stream, [&] { return e->set_hint(cn, hint, B, Hh, Wh); });
}

int fgdm_set_concat(fgdm_engine* e, const float* c_concat, int B, int Cc, int H, int W, void* stream) {
    if (!e) return FGDM_ERR_ARG;
    return stream_call(e, stream, [&] { return e->set_concat(c_concat, B, Cc, H, W); });
}

int fgdm_apply_model(fgdm_engine* e, const float* x, const int64_t* t, const float* t_float, const float* ctx,
                     const float* pcond, const float* control_scales, int B, int H, int W, int flags, float* eps_out,
                     void* stream) {
    if (!e || !x || (!t && !t_float) || !eps_out) return FGDM_ERR_ARG;
    return stream_call(e, stream, [&] { return e->apply_model(x, t, t_float, ctx, pcond, control_scales, B, H, W, flags, eps_out); });
}

int fgdm_set_adapter_conds(fgdm_engine* e, const float* const* conds, int n_conds, int B, int H, int W, void* stream) {
    if (!e) return FGDM_ERR_ARG;
    return stream_call(e, stream, [&] { return e->set_adapter_conds(conds, n_conds, B, H, W); });
}

int fgdm_set_context(fgdm_engine* e, const float* ctx, int B, void* stream) {
    if (!e || !ctx) return FGDM_ERR_ARG;
    return stream_call(e, stream, [&] { return e->set_context(ctx, B); });
}

int fgdm_clip_encode(fgdm_engine* e, const int64_t* ids, int B, int T, float* out, void* stream) {
    if (!e || !ids || !out) return FGDM_ERR_ARG;
    return stream_call(e, stream, [&] { return e->clip_encode(ids, B, T, out); });
}

int fgdm_clip_encode_skip(fgdm_engine* e, const int64_t* ids, int B, int T, int clip_skip, float* out, void* stream) {
    if (!e || !ids || !out) return FGDM_ERR_ARG;
    return stream_call(e, stream, [&] { return e->clip_encode(ids, B, T, out, clip_skip); });
}

int fgdm_set_context_tokens(fgdm_engine* e, int tokens) {
    if (!e) return FGDM_ERR_ARG;
    if (tokens < 1) return e->fail(FGDM_ERR_ARG, "context token count must be >= 1");
    if (tokens != e->ctx_tokens) { e->drop_context(); e->ctx_tokens = tokens; }      // cached projections have the old length
    return FGDM_OK;
}

int fgdm_get_context_tokens(const fgdm_engine* e) { return e ? e->ctx_tokens : FGDM_ERR_ARG; }

// ------------------------------------------------------------------------------------------------ cross-attention maps
int fgdm_attention_capture_set(fgdm_engine* e, const fgdm_attention_capture* plan) {
    if (!e) return FGDM_ERR_ARG;
    if (!plan) { e->capture_off(); return FGDM_OK; }
    fgdm_attention_capture p;
    if (!read_params(plan, FGDM_ATTENTION_CAPTURE_SIZE_V1, &p, sizeof(p)))
        return e->fail(FGDM_ERR_ARG, "attention capture: struct_size is not the sizeof(fgdm_attention_capture) of a known header version");
    if (p.reserved0) return e->fail(FGDM_ERR_ARG, "attention capture: reserved0 must be 0");
    if (!e->finalized) return e->fail(FGDM_ERR_STATE, "weights not finalized");
    std::vector<const Layer*> order;
    for_each_block(e->unet, false, [&](const Block& blk) {
        for (const Layer& l : blk) if (l.type == L_ATTN) order.push_back(&l);
        return FGDM_OK;
    });
    const int nb = (int)order.size(), Tk = e->ctx_tokens;
    if (!p.block_mask || (nb < 32 && (p.block_mask >> nb)))
        return e->fail(FGDM_ERR_ARG, "attention capture: block_mask must name at least one of the UNet's " + std::to_string(nb) + " transformer blocks and no other");
    if (Tk > FGDM_ATTENTION_CAPTURE_MAX_KEYS)
        return e->fail(FGDM_ERR_ARG, "attention capture: the context has " + std::to_string(Tk) + " tokens, more than FGDM_ATTENTION_CAPTURE_MAX_KEYS, the capturing kernels' key limit");
    if (Tk >= 128 && Tk % 64 == 0)
        return e->fail(FGDM_ERR_ARG, "attention capture: a context of 128, 192 or 256 tokens runs on the self-attention kernels, which have no capturing form");
    if (p.n_tokens < 0 || p.n_tokens > Tk || (p.n_tokens > 0 && !p.tokens))
        return e->fail(FGDM_ERR_ARG, "attention capture: n_tokens must lie in [0, context tokens], with tokens given when it is not 0");
    std::vector<int> tokens;
    for (int i = 0; i < (p.n_tokens ? p.n_tokens : Tk); ++i) {
        const int k = p.n_tokens ? p.tokens[i] : i;
        if (k < 0 || k >= Tk) return e->fail(FGDM_ERR_ARG, "attention capture: token index " + std::to_string(k) + " is outside the registered context of " + std::to_string(Tk) + " tokens");
        tokens.push_back(k);
    }
    if (p.rows < FGDM_CAPTURE_ROWS_ALL || p.rows > FGDM_CAPTURE_ROWS_UNCOND) return e->fail(FGDM_ERR_ARG, "attention capture: rows must be FGDM_CAPTURE_ROWS_ALL, _COND or _UNCOND");
    if (p.mode != FGDM_CAPTURE_SUM && p.mode != FGDM_CAPTURE_LAST) return e->fail(FGDM_ERR_ARG, "attention capture: mode must be FGDM_CAPTURE_SUM or FGDM_CAPTURE_LAST");
    const bool sized = p.batch > 0 && p.latent_h > 0 && p.latent_w > 0;
    if (!sized && (p.batch || p.latent_h || p.latent_w))
        return e->fail(FGDM_ERR_ARG, "attention capture: batch, latent_h and latent_w must be all positive or all 0");
    if (sized && p.rows != FGDM_CAPTURE_ROWS_ALL && (p.batch & 1))
        return e->fail(FGDM_ERR_ARG, "attention capture: the conditional / unconditional half of an odd batch");
    e->capture_off();
    auto& c = e->cap;
    c.rows_sel = p.rows; c.mode = p.mode; c.Tk = Tk;
    c.tokens = tokens; c.order = order;
    for (int i = 0; i < nb; ++i)
        if ((p.block_mask >> i) & 1) { fgdm_engine::CapPlane pl; pl.block = i; c.planes[order[i]] = pl; }
    if (sized) {
        const int rc = e->capture_alloc(p.batch, p.latent_h, p.latent_w);
        if (rc != FGDM_OK) { e->capture_off(); return rc; }
    }
    c.on = true;
    return FGDM_OK;
}
// ------------------------------------------------------------------------------------------------ device noise
int fgdm_loop_noise_set(fgdm_engine* e, const fgdm_noise_plan* plan) {
    if (!e) return FGDM_ERR_ARG;
    if (!plan) { e->loop_noise = fgdm_engine::LoopNoise{}; return FGDM_OK; }
    fgdm_noise_plan p;
    if (!read_params(plan, FGDM_NOISE_PLAN_SIZE_V1, &p, sizeof(p)))
        return e->fail(FGDM_ERR_ARG, "loop noise: struct_size is not the sizeof(fgdm_noise_plan) of a known header version");
    if (p.reserved0 || p.reserved1) return e->fail(FGDM_ERR_ARG, "loop noise: reserved0 and reserved1 must be 0");
    if (p.first_sample < 0 || p.first_step < 0) return e->fail(FGDM_ERR_ARG, "loop noise: first_sample and first_step must not be negative");
    uint32_t tbits;                     // by the exponent field: this file is compiled with -fno-honor-nans
    memcpy(&tbits, &p.temperature, sizeof(tbits));
    if ((tbits & 0x7F800000u) == 0x7F800000u) return e->fail(FGDM_ERR_ARG, "loop noise: temperature must be finite");
    auto& n = e->loop_noise;
    n.on = true; n.seed = p.seed; n.first_sample = p.first_sample; n.first_step = p.first_step;
    n.temperature = p.temperature; n.repeat = p.repeat_noise != 0;
    return FGDM_OK;
}
int fgdm_randn(uint64_t seed, int32_t stream_id, int32_t step, int32_t first_sample, int32_t repeat, float temperature, float* out,
               int32_t B, int32_t per_sample, void* stream) {
    if (stream_id < 0 || step < 0 || first_sample < 0 || per_sample <= 0 || B <= 0 || (int64_t)first_sample + B - 1 > INT32_MAX)
        return FGDM_ERR_ARG;
    return randn_fill(seed, (uint32_t)stream_id, (uint32_t)step, (uint32_t)first_sample, repeat != 0, temperature, out, B,
                      (uint32_t)per_sample, as_stream(stream));
}

static const fgdm_engine::CapPlane* capture_block(fgdm_engine* e, int block) {
    if (!e->cap.on || block < 0 || block >= (int)e->cap.order.size()) return nullptr;
    auto it = e->cap.planes.find(e->cap.order[block]);
    return it == e->cap.planes.end() ? nullptr : &it->second;
}
int fgdm_attention_capture_reset(fgdm_engine* e, void* stream) {
    if (!e) return FGDM_ERR_ARG;
    if (!e->cap.on) return e->fail(FGDM_ERR_STATE, "attention capture is off");
    e->cap.n_evals = 0;
    for (auto& kv : e->cap.planes)
        if (kv.second.acc && hipMemsetAsync(kv.second.acc, 0, e->capture_plane_floats(kv.second) * sizeof(float), as_stream(stream)) != hipSuccess)
            return e->fail(FGDM_ERR_HIP, "hipMemsetAsync (attention capture)");
    return FGDM_OK;
}
int fgdm_attention_capture_info(fgdm_engine* e, int block, int64_t shape[3], int32_t* n_evals) {
    if (!e) return FGDM_ERR_ARG;
    const auto* p = capture_block(e, block);
    if (!p) return e->fail(FGDM_ERR_ARG, "attention capture: block " + std::to_string(block) + " is not selected");
    if (shape) { shape[0] = e->cap.B ? e->cap.rows : 0; shape[1] = (int64_t)p->h * p->w; shape[2] = e->cap.B ? (int64_t)e->cap.tokens.size() : 0; }
    if (n_evals) *n_evals = e->cap.n_evals;
    return FGDM_OK;
}
int fgdm_attention_capture_block_size(fgdm_engine* e, int block, int32_t* h, int32_t* w) {
    if (!e || !h || !w) return FGDM_ERR_ARG;
    const auto* p = capture_block(e, block);
    if (!p) return e->fail(FGDM_ERR_ARG, "attention capture: block " + std::to_string(block) + " is not selected");
    *h = p->h; *w = p->w;
    return FGDM_OK;
}
int fgdm_attention_capture_read(fgdm_engine* e, int block, float* dst_device, void* stream) {
    if (!e || !dst_device) return FGDM_ERR_ARG;
    const auto* p = capture_block(e, block);
    if (!p) return e->fail(FGDM_ERR_ARG, "attention capture: block " + std::to_string(block) + " is not selected");
    if (!p->acc) return e->fail(FGDM_ERR_STATE, "attention capture: no evaluation has been captured yet");
    if (hipMemcpyAsync(dst_device, p->acc, e->capture_plane_floats(*p) * sizeof(float), hipMemcpyDeviceToDevice, as_stream(stream)) != hipSuccess)
        return e->fail(FGDM_ERR_HIP, "hipMemcpyAsync (attention capture)");
    return FGDM_OK;
}

int fgdm_vae_decode(fgdm_engine* e, const float* z, int B, int H, int W, float scale, float* image, void* stream) {
    if (!e || !z || !image) return FGDM_ERR_ARG;
    return stream_call(e, stream, [&] { return e->vae_decode(z, B, H, W, scale, image); });
}

int fgdm_vae_encode(fgdm_engine* e, const float* image, int B, int H, int W, float* moments, void* stream) {
    if (!e || !image || !moments) return FGDM_ERR_ARG;
    return stream_call(e, stream, [&] { return e->vae_encode(image, B, H, W, moments); });
}
int fgdm_posterior_sample(const float* moments, const float* noise, float scale, float* z, int B, int zc, int HW, void* stream) {
    if (!moments || !z || B <= 0 || zc <= 0 || HW <= 0) return FGDM_ERR_ARG;
    return posterior_sample(moments, noise, scale, z, B, zc, HW, as_stream(stream));
}

// ---- patch-wise routes (split_input_params; kernels in patches.hip).  Argument errors come before any launch.
int fgdm_vae_decode_patches(fgdm_engine* e, const float* z, int B, int H, int W, float scale, int kh, int kw, int sh, int sw,
                            int f, const float* w_pix, const float* w_tie, int max_crops_per_pass, float* image, void* stream) {
    if (!e) return FGDM_ERR_ARG;
    if (!z || !w_pix || !w_tie || !image || B <= 0 || max_crops_per_pass < 0) return e->fail(FGDM_ERR_ARG, "patch decode: null pointer or bad batch / pass size");
    if (!e->vae.on) return e->fail(FGDM_ERR_STATE, "engine was created without a first-stage decoder (vae_ch = 0)");
    if (!e->comps[e->vae_comp].packed) return e->fail(FGDM_ERR_STATE, "weights not finalized");
    if (f != e->vae.factor) return e->fail(FGDM_ERR_ARG, "patch decode: f (vqf) must equal the decoder's upscaling factor " + std::to_string(e->vae.factor));
    PatchGeom gz{B, 4, H, W, kh, kw, sh, sw, 0, 0};
    if (patch_plan(H, W, kh, kw, sh, sw, true, &gz.Ly, &gz.Lx) != FGDM_OK)
        return e->fail(FGDM_ERR_ARG, "patch decode: the crops do not cover the latent grid ((size - ks) % stride != 0, stride > ks or ks > size)");
    if ((kh * kw) & 63) return e->fail(FGDM_ERR_ARG, "patch decode: kh * kw must be a multiple of 64 (first-stage attention)");
    const int oc = e->cfg.vae_out_ch, L = gz.Ly * gz.Lx;
    const PatchGeom gi{B, oc, H * f, W * f, kh * f, kw * f, sh * f, sw * f, gz.Ly, gz.Lx};
    int step = std::min(max_crops_per_pass, L);
    if (step == 0) {      // fgdm_vae_decode's images-per-pass rule, applied to the L * B crop images
        const size_t big = (size_t)gi.kh * gi.kw * e->cfg.vae_ch * sizeof(half_t) * 8;
        const size_t imgs = std::max<size_t>(1, std::min<size_t>((size_t)L * B, ((size_t)3 << 30) / std::max<size_t>(big, 1)));
        step = (int)std::max<size_t>(1, std::min<size_t>((size_t)L, imgs / (size_t)B));
    }
    return stream_call(e, stream, [&]() -> int {
        const size_t zc_n = (size_t)B * 4 * kh * kw, oc_n = (size_t)B * oc * gi.kh * gi.kw;
        Buf zc_buf, ocr_buf;
        CHK(e->balloc(&zc_buf, (size_t)step * zc_n * sizeof(float)));
        CHK(e->balloc(&ocr_buf, (size_t)step * oc_n * sizeof(float)));
        float *const zc = zc_buf.as<float>(), *const ocr = ocr_buf.as<float>();
        for (int l0 = 0; l0 < L; l0 += step) {
            const int n = std::min(step, L - l0);
            if (unfold_crops(z, zc, gz, l0, n, e->s) != FGDM_OK) return e->fail(FGDM_ERR_HIP, "unfold kernel");
            CHK(e->vae_decode(zc, n * B, kh, kw, scale, ocr));
            if (fold_accumulate(ocr, w_pix, w_tie, image, gi, l0, n, e->s) != FGDM_OK) return e->fail(FGDM_ERR_HIP, "fold kernel");
        }
        if (fold_finish(image, w_pix, w_tie, image, gi, e->s) != FGDM_OK) return e->fail(FGDM_ERR_HIP, "fold kernel");
        return FGDM_OK;
    });
}

int fgdm_apply_model_patches(fgdm_engine* e, const float* x, const int64_t* t, const float* t_float, const float* ctx, int B,
                             int H, int W, int kh, int kw, int sh, int sw, const float* w_pix, const float* w_tie,
                             int max_crops_per_pass, int flags, float* eps_out, void* stream) {
    if (!e) return FGDM_ERR_ARG;
    if (!x || (!t && !t_float) || !w_pix || !w_tie || !eps_out || B <= 0 || max_crops_per_pass < 0)
        return e->fail(FGDM_ERR_ARG, "patch apply_model: null pointer or bad batch / pass size");
    if (!ctx) return e->fail(FGDM_ERR_ARG, "patch apply_model: ctx must be given (a registered context covers B rows, a pass has n*B)");
    if (!e->cns.empty()) return e->fail(FGDM_ERR_ARG, "patch apply_model: ControlLDM.apply_model has no patch branch (engine has ControlNets)");
    if (e->cfg.in_channels != 4)
        return e->fail(FGDM_ERR_ARG, "patch apply_model: in_channels != 4 -- the reference crops c_concat only for its spatial cond_stage_keys "
                                     "(ddpm.py:1061-1071), which are refused");
    if (!e->finalized) return e->fail(FGDM_ERR_STATE, "weights not finalized");
    PatchGeom g{B, 4, H, W, kh, kw, sh, sw, 0, 0};
    if (patch_plan(H, W, kh, kw, sh, sw, true, &g.Ly, &g.Lx) != FGDM_OK)
        return e->fail(FGDM_ERR_ARG, "patch apply_model: the crops do not cover the latent grid ((size - ks) % stride != 0, stride > ks or ks > size)");
    const int L = g.Ly * g.Lx, step = max_crops_per_pass > 0 ? std::min(max_crops_per_pass, L) : L;
    const int fl = (flags & FGDM_FLAG_USE_ORIGINAL) | FGDM_FLAG_NO_CONTROL;      // CFG_PAIRS cleared: rows are (l, b)
    return stream_call(e, stream, [&]() -> int {
        const size_t xc_n = (size_t)B * 4 * kh * kw, ctx_n = (size_t)B * e->ctx_tokens * e->cfg.context_dim;
        Buf xc_buf, ec_buf, cr_buf, tr_buf;
        CHK(e->balloc(&xc_buf, (size_t)step * xc_n * sizeof(float)));
        CHK(e->balloc(&ec_buf, (size_t)step * xc_n * sizeof(float)));
        CHK(e->balloc(&cr_buf, (size_t)step * ctx_n * sizeof(float)));
        CHK(e->balloc(&tr_buf, (size_t)step * B * sizeof(int64_t)));
        float *const xc = xc_buf.as<float>(), *const ec = ec_buf.as<float>(), *const cr = cr_buf.as<float>();
        void* const tr = tr_buf.p;
        // t and the context of every crop (ddpm.py:1116,1119); a shorter last pass reads a prefix of the same buffers
        if (repeat_words(ctx, cr, ctx_n, step, e->s) != FGDM_OK ||
            repeat_words(t_float ? (const void*)t_float : (const void*)t, tr, t_float ? (size_t)B : (size_t)2 * B, step, e->s) != FGDM_OK)
            return e->fail(FGDM_ERR_HIP, "repeat kernel");
        for (int l0 = 0; l0 < L; l0 += step) {
            const int n = std::min(step, L - l0);
            if (unfold_crops(x, xc, g, l0, n, e->s) != FGDM_OK) return e->fail(FGDM_ERR_HIP, "unfold kernel");
            CHK(e->apply_model(xc, t_float ? nullptr : (const int64_t*)tr, t_float ? (const float*)tr : nullptr, cr, nullptr, nullptr,
                               n * B, kh, kw, fl, ec));
            if (fold_accumulate(ec, w_pix, w_tie, eps_out, g, l0, n, e->s) != FGDM_OK) return e->fail(FGDM_ERR_HIP, "fold kernel");
        }
        if (fold_finish(eps_out, w_pix, w_tie, eps_out, g, e->s) != FGDM_OK) return e->fail(FGDM_ERR_HIP, "fold kernel");
        return FGDM_OK;
    });
}

int fgdm_controlnet(fgdm_engine* e, int cn, const float* x, const int64_t* t, const float* ctx, int B, int H, int W,
                    float* out, int64_t out_capacity_floats, void* stream) {
    if (!e || !x || !t || !ctx || !out) return FGDM_ERR_ARG;
    if (!e->finalized) return e->fail(FGDM_ERR_STATE, "weights not finalized");
    if (cn < 0 || cn >= (int)e->cns.size()) return e->fail(FGDM_ERR_ARG, "no such ControlNet");
    return stream_call(e, stream, [&]() -> int {
        fgdm_engine::Act x4, ctx16;
        CHK(e->talloc(&x4, B, H, W, 4));
        CHK(e->talloc(&ctx16, B, 1, e->ctx_tokens, e->cfg.context_dim));
        if (nchw_f32_to_nhwc_f16(x, x4.p, B, 4, H * W, 4, e->s) != FGDM_OK) return e->fail(FGDM_ERR_HIP, "layout kernel");
        if (f32_to_f16(ctx, ctx16.p, ctx16.numel(), e->s) != FGDM_OK) return e->fail(FGDM_ERR_HIP, "convert kernel");
        return e->controlnet_fwd(e->cns[cn], x4, t, nullptr, ctx16, nullptr, nullptr, nullptr, false, out, out_capacity_floats);
    });
}

int fgdm_run_block(fgdm_engine* e, const char* prefix, const float* x, int C, const float* x_skip, int Cs, const float* emb,
                   const float* ctx, int B, int H, int W, float* out, int64_t out_capacity_floats, int64_t* out_numel,
                   void* stream) {
    if (!e || !prefix || !x || !out) return FGDM_ERR_ARG;
    return stream_call(e, stream, [&] { return e->run_block(prefix, x, C, x_skip, Cs, emb, ctx, B, H, W, out, out_capacity_floats, out_numel); });
}

int fgdm_ddim_step(const float* x, const float* e_cond, const float* e_uncond, float cfg_scale, float a_t, float a_prev,
                   float sigma_t, float sqrt_one_minus_at, const float* noise, float* x_prev, float* pred_x0,
                   float* e_out, int64_t n, void* stream) {
    if (!x || !e_cond || n <= 0) return FGDM_ERR_ARG;
    return ddim_step(x, e_cond, e_uncond, cfg_scale, a_t, a_prev, sigma_t, sqrt_one_minus_at, noise, x_prev, pred_x0,
                     e_out, (size_t)n, as_stream(stream));
}
int fgdm_plms_combine(const float* e_t, const float* e1, const float* e2, const float* e3, int order, float* e_prime,
                      int64_t n, void* stream) {
    if (!e_t || !e_prime || n <= 0) return FGDM_ERR_ARG;
    return plms_combine(e_t, e1, e2, e3, order, e_prime, (size_t)n, as_stream(stream));
}
int fgdm_axpby(const float* a, float ca, const float* b, float cb, float* y, int64_t n, void* stream) {
    if (!a || !y || n <= 0) return FGDM_ERR_ARG;
    return axpby(a, ca, b, cb, y, (size_t)n, as_stream(stream));
}
int fgdm_mask_blend(const float* a, const float* b, const float* mask, float* y, int64_t n, void* stream) {
    if (!a || !b || !mask || !y || n <= 0) return FGDM_ERR_ARG;
    return mask_blend(a, b, mask, y, (size_t)n, as_stream(stream));
}
int fgdm_ancestral_step(const float* x, const float* eps, float sqrt_recip_ac, float sqrt_recipm1_ac, float coef1,
                        float coef2, float std, const float* noise, float* out, int64_t n, void* stream) {
    if (!x || !eps || !out || n <= 0) return FGDM_ERR_ARG;
    return ancestral_step(x, eps, sqrt_recip_ac, sqrt_recipm1_ac, coef1, coef2, std, noise, out, (size_t)n, as_stream(stream));
}

int fgdm_image_to_uint8(const float* image, int B, int C, int H, int W, int mode, uint8_t* out, void* stream) {
    if (!image || !out) return FGDM_ERR_ARG;
    return image_to_u8(image, out, B, C, H * W, mode, as_stream(stream));
}
int fgdm_resize_linear_uint8(const uint8_t* src, int B, int H, int W, int C, int Ho, int Wo, uint8_t* dst, void* stream) {
    if (!src || !dst) return FGDM_ERR_ARG;
    return resize_linear_u8(src, dst, B, H, W, C, Ho, Wo, as_stream(stream));
}
int fgdm_uint8_to_hint(const uint8_t* src, int B, int H, int W, int C, float* hint, void* stream) {
    if (!src || !hint) return FGDM_ERR_ARG;
    return u8_to_hint(src, hint, B, H * W, C, as_stream(stream));
}

// ---- the device sampler loops (fgdm_sample_ddim_ex, fgdm_sample_plms, fgdm_sample_dpmpp, fgdm_sample_dpm_solver, ...)
// A walk of the DDIM family, as fgdm_sample_ddim_ex and fgdm_sample_plms fill it from their public structs: the fields the two
// share by name (walk_from), the DDIM entry's sigmas / step_noise / cfg_scales (NULL: absent), and what the entry has resolved:
// cfg_on (one decision for the whole walk: the registered context has Bm rows), the flags of every evaluation, and `plms`.
struct Walk {
    float* x;
    const float *cond, *uncond;
    const int64_t* timesteps;
    const float *alphas, *alphas_prev, *sqrt_one_minus_alphas, *control_scales;
    const float *sigmas, *step_noise, *cfg_scales;
    const float *mask, *x0, *q_noise, *sqrt_alphas_cumprod_t, *sqrt_one_minus_alphas_cumprod_t;
    const int32_t* log_steps;
    float *x_inter_out, *pred_x0_out;
    float cfg_scale;
    int S, B, H, W, flags, n_log, reserved0;
    bool cfg_on, plms;
};
extern "C++" template <typename P> static Walk walk_from(const P& p) {
    Walk w{};
    w.x = p.x; w.cond = p.cond; w.uncond = p.uncond; w.timesteps = p.timesteps;
    w.alphas = p.alphas; w.alphas_prev = p.alphas_prev; w.sqrt_one_minus_alphas = p.sqrt_one_minus_alphas;
    w.control_scales = p.control_scales;
    w.mask = p.mask; w.x0 = p.x0; w.q_noise = p.q_noise;
    w.sqrt_alphas_cumprod_t = p.sqrt_alphas_cumprod_t; w.sqrt_one_minus_alphas_cumprod_t = p.sqrt_one_minus_alphas_cumprod_t;
    w.log_steps = p.log_steps; w.x_inter_out = p.x_inter_out; w.pred_x0_out = p.pred_x0_out;
    w.cfg_scale = p.cfg_scale; w.S = p.S; w.B = p.B; w.H = p.H; w.W = p.W; w.flags = p.flags; w.n_log = p.n_log;
    w.reserved0 = p.reserved0;
    return w;
}
// The log_steps of every loop's struct: strictly ascending walk positions in [0, S).
static const char* log_steps_error(const int32_t* log_steps, int n_log, int S) {
    if (n_log < 0 || (n_log > 0 && !log_steps)) return "n_log < 0, or log steps without log_steps";
    for (int j = 0; j < n_log; ++j)
        if (log_steps[j] < 0 || log_steps[j] >= S || (j > 0 && log_steps[j] <= log_steps[j - 1]))
            return "log_steps must be strictly ascending walk positions in [0, S)";
    return nullptr;
}
// Host-side checks of a walk, in front of any launch; nullptr: the parameters are consistent.
// The sample and step ranges of an armed call: global sample indices and walk positions are 32-bit counter words (noise.h).
static const char* loop_noise_range_error(const fgdm_engine* e, int B, int S) {
    const auto& n = e->loop_noise;
    if ((int64_t)n.first_sample + B > INT32_MAX || (int64_t)n.first_step + S > INT32_MAX)
        return "loop noise: first_sample + B and first_step + S must not exceed INT32_MAX";
    return nullptr;
}
static const char* walk_error(const Walk& p, const fgdm_engine* e) {
    const bool armed = e->loop_noise.on;
    if (p.reserved0 != 0) return "reserved0 must be 0";
    if (!p.x || !p.cond || !p.timesteps || !p.alphas || !p.alphas_prev || !p.sqrt_one_minus_alphas) return "x, cond or a schedule table is NULL";
    if (p.S <= 0 || p.B <= 0 || p.H <= 0 || p.W <= 0) return "S, B, H and W must be positive";
    if (p.mask && (!p.x0 || (!p.q_noise && !armed) || !p.sqrt_alphas_cumprod_t || !p.sqrt_one_minus_alphas_cumprod_t))
        return "mask needs x0, q_noise and q_sample's two coefficient tables";
    if (p.sigmas && !p.step_noise && !armed)
        for (int k = 0; k < p.S; ++k)
            if (p.sigmas[k] != 0.f) return "a sigma is not 0 and step_noise is NULL";
    if (armed)
        if (const char* why = loop_noise_range_error(e, p.B, p.S)) return why;
    return log_steps_error(p.log_steps, p.n_log, p.S);
}

// The walk itself (inside the entry's stream_call): per step one evaluation of the network on cat([x] * 2) (or x, CFG off), then
// one launch of k_loop_step, which also does the NEXT step's blend and writes x into the network's input.  PLMS (plms.py:178-236)
// differs in the three history planes, the probe and the second evaluation of the first step, and the mode / order of the launch.
static int run_walk(fgdm_engine* e, const Walk& p, hipStream_t s) {
    const int S = p.S;
    Loop L(e, s, p, S, p.cfg_on, p.flags, p.log_steps, p.n_log);
    CHK(L.begin(p.cond, p.uncond, p.timesteps, nullptr, p.plms ? 3 : 0));      // PLMS: e_t of step j lives in plane j % 3
    const size_t n = L.n;
    auto plane = [&](int step) { return L.plane(step % 3); };
    // the blend in front of step `i` (index k = S - 1 - i), done by the kernel of the step before it
    auto blend = [&](LoopStep& a, int i) {
        if (!p.mask) return;
        const int k = S - 1 - i;
        a.mask = p.mask; a.x0 = p.x0; a.qnoise = p.q_noise ? p.q_noise + (size_t)i * n : nullptr;
        a.sa_next = p.sqrt_alphas_cumprod_t[k]; a.s1m_next = p.sqrt_one_minus_alphas_cumprod_t[k];
    };
    // what the launch behind step `i` makes itself while the engine is armed: its sigma * noise where no plane is given, and the
    // q_sample noise of the blend in front of step `qi` (-1: no blend in this launch) likewise
    auto gen = [&](const LoopStep& a, int i, int qi) {
        return e->noise_gen(p.H, p.W, i, qi < 0 ? 0 : qi, i >= 0 && a.sigma != 0.f && !a.noise, qi >= 0 && a.mask && !a.qnoise);
    };
    int rc;
    {                                   // in front of the first step: its blend, and x into the network's input
        LoopStep a{};
        a.io.x = L.x; a.io.n = n; L.feed(a.io);
        blend(a, 0);
        a.gen = gen(a, -1, 0);
        a.io.x_out = p.mask ? L.x : nullptr;
        rc = loop_step(a, s);
    }
    for (int i = 0; i < S && rc == FGDM_OK; ++i) {
        const int index = S - 1 - i;   // reversed walk (ddim.py:137,148; plms.py:138,150)
        rc = L.eval(index);
        if (rc != FGDM_OK) break;
        LoopStep a{};
        a.io = L.step_io(i, p.cfg_scales ? p.cfg_scales[i] : p.cfg_scale);
        a.a_t = p.alphas[index]; a.a_prev = p.alphas_prev[index]; a.s1m = p.sqrt_one_minus_alphas[index];
        a.sigma = p.sigmas ? p.sigmas[index] : 0.f;
        a.noise = a.sigma != 0.f && p.step_noise ? p.step_noise + (size_t)i * n : nullptr;
        a.gen = gen(a, i, -1);
        if (!p.plms) {
            a.mode = LOOP_PLAIN;
        } else if (i == 0) {            // pseudo improved Euler (plms.py:219-223): probe, second evaluation at t_next, finish
            LoopStep probe = a;
            probe.mode = LOOP_PROBE; probe.e_out = plane(0); L.feed(probe.io);
            rc = loop_step(probe, s);
            if (rc == FGDM_OK) rc = L.eval(S >= 2 ? S - 2 : 0);
            if (rc != FGDM_OK) break;
            a.mode = LOOP_FINISH_FIRST; a.e1 = plane(0);
        } else {                        // Adams-Bashforth over the last min(i, 3) planes (plms.py:224-232)
            a.mode = LOOP_MULTISTEP; a.order = i < 3 ? i : 3;
            a.e_out = plane(i); a.e1 = plane(i - 1);
            if (i >= 2) a.e2 = plane(i - 2);
            if (i >= 3) a.e3 = plane(i - 3);      // the plane e_out replaces
        }
        if (i + 1 < S) { blend(a, i + 1); a.gen = gen(a, i, i + 1); }
        const int slot = L.log_slot(i);
        a.io.log_x = L.log_plane(p.x_inter_out, slot); a.log_p0 = L.log_plane(p.pred_x0_out, slot);
        rc = loop_step(a, s);
    }
    return rc;
}

static Walk ddim_walk(const fgdm_ddim_params& known) {
    Walk p = walk_from(known);
    p.sigmas = known.sigmas; p.step_noise = known.step_noise; p.cfg_scales = known.cfg_scales;
    return p;
}
// This entry takes hybrid networks, and the flags go to the network as given; CFG is on when any step's scale is not 1
int fgdm_sample_ddim_ex(fgdm_engine* e, const fgdm_ddim_params* caller, void* stream) {
    return loop_entry(e, caller, stream, FGDM_DDIM_PARAMS_SIZE_V1, "fgdm_sample_ddim_ex", "fgdm_ddim_params", false,
                      [e](const fgdm_ddim_params& known) { return walk_error(ddim_walk(known), e); },
                      [](fgdm_engine* e, const fgdm_ddim_params& known, hipStream_t s) {
                          Walk p = ddim_walk(known);
                          if (p.uncond)
                              for (int i = 0; i < p.S && !p.cfg_on; ++i) p.cfg_on = (p.cfg_scales ? p.cfg_scales[i] : p.cfg_scale) != 1.0f;
                          return run_walk(e, p, s);
                      });
}

int fgdm_sample_ddim(fgdm_engine* e, float* x, const float* cond, const float* uncond, float cfg_scale, int S,
                     const int64_t* timesteps, const float* alphas, const float* alphas_prev,
                     const float* sqrt_one_minus_alphas, const float* control_scales, int B, int H, int W, int flags,
                     void* stream) {
    if (!e || !x || !cond || !timesteps || !alphas || !alphas_prev || !sqrt_one_minus_alphas || S <= 0) return FGDM_ERR_ARG;
    fgdm_ddim_params p{};
    p.struct_size = sizeof(p);
    p.x = x; p.cond = cond; p.uncond = uncond; p.cfg_scale = cfg_scale; p.S = S; p.timesteps = timesteps;
    p.alphas = alphas; p.alphas_prev = alphas_prev; p.sqrt_one_minus_alphas = sqrt_one_minus_alphas;
    p.control_scales = control_scales; p.B = B; p.H = H; p.W = W; p.flags = flags;
    return fgdm_sample_ddim_ex(e, &p, stream);
}

int fgdm_sample_plms(fgdm_engine* e, const fgdm_plms_params* caller, void* stream) {
    return loop_entry(e, caller, stream, FGDM_PLMS_PARAMS_SIZE_V1, "fgdm_sample_plms", "fgdm_plms_params", true,
                      [e](const fgdm_plms_params& known) { return walk_error(walk_from(known), e); },
                      [](fgdm_engine* e, const fgdm_plms_params& known, hipStream_t s) {
                          Walk p = walk_from(known);
                          p.plms = true;
                          p.cfg_on = loop_cfg_on(p.uncond, p.cfg_scale);
                          p.flags = loop_flags(p.flags, p.cfg_on);
                          return run_walk(e, p, s);
                      });
}

static const char* dpmpp_params_error(const fgdm_dpmpp_params* p) {
    if (p->reserved0 != 0 || p->reserved1 != 0) return "reserved0 and reserved1 must be 0";
    if (!p->x || !p->cond || !p->t_float || !p->inv_alpha || !p->neg_sigma_over_alpha || !p->update_kind || !p->c1 || !p->cm0 || !p->cm1)
        return "x, cond or a table is NULL";
    if (p->n_eval <= 0 || p->B <= 0 || p->H <= 0 || p->W <= 0) return "n_eval, B, H and W must be positive";
    for (int k = 0; k < p->n_eval; ++k)
        if (p->update_kind[k] != FGDM_DPMPP_FIRST && p->update_kind[k] != FGDM_DPMPP_SECOND)
            return "update_kind must be FGDM_DPMPP_FIRST or FGDM_DPMPP_SECOND";
    if (p->update_kind[0] == FGDM_DPMPP_SECOND) return "update_kind[0] is second-order: there is no earlier data prediction";
    return nullptr;
}

static int run_dpmpp(fgdm_engine* e, const fgdm_dpmpp_params& p, hipStream_t s) {
    const int K = p.n_eval;
    const bool cfg_on = loop_cfg_on(p.uncond, p.cfg_scale);
    Loop L(e, s, p, K, cfg_on, loop_flags(p.flags, cfg_on));
    CHK(L.begin(p.cond, p.uncond, nullptr, p.t_float, 2));      // the data prediction of evaluation k lives in plane k % 2
    CHK(L.seed());
    int rc = FGDM_OK;
    for (int k = 0; k < K && rc == FGDM_OK; ++k) {
        rc = L.eval(k);
        if (rc != FGDM_OK) break;
        DpmppLoopStep a{};
        a.io = L.step_io(k, p.cfg_scale);
        a.inv_alpha = p.inv_alpha[k]; a.neg_sigma_over_alpha = p.neg_sigma_over_alpha[k];
        a.kind = p.update_kind[k]; a.c1 = p.c1[k]; a.cm0 = p.cm0[k]; a.cm1 = p.cm1[k];
        a.m0_out = L.plane(k % 2);
        a.m1 = k > 0 ? L.plane((k - 1) % 2) : nullptr;
        rc = dpmpp_loop_step(a, s);
    }
    return rc;
}
int fgdm_sample_dpmpp(fgdm_engine* e, const fgdm_dpmpp_params* caller, void* stream) {
    return loop_entry(e, caller, stream, FGDM_DPMPP_PARAMS_SIZE_V1, "fgdm_sample_dpmpp", "fgdm_dpmpp_params", true,
                      [](const fgdm_dpmpp_params& known) { return dpmpp_params_error(&known); }, run_dpmpp);
}

// The checks of a DPM-Solver program, in front of any launch; empty: the program is consistent.
static std::string dpm_program_error(const fgdm_dpm_solver_params* p) {
    if (p->reserved0 != 0 || p->reserved1 != 0) return "reserved0 and reserved1 must be 0";
    if (!p->x || !p->cond || !p->t_float || !p->conv_x || !p->conv_e || !p->slot || !p->nterms || !p->plane || !p->coef || !p->dest)
        return "x, cond or a program array is NULL";
    if (p->n_eval <= 0 || p->B <= 0 || p->H <= 0 || p->W <= 0) return "n_eval, B, H and W must be positive";
    bool written[3] = {false, false, false};
    for (int k = 0; k < p->n_eval; ++k) {
        const std::string rec = "record " + std::to_string(k) + ": ";
        const int nt = p->nterms[k];
        if (nt < 1 || nt > DPM_MAX_TERMS) return rec + "nterms " + std::to_string(nt) + " is outside 1..5";
        for (int j = 0; j < nt; ++j) {
            const int src = p->plane[(size_t)k * DPM_MAX_TERMS + j];
            if (src < FGDM_DPM_PLANE_BASE || src > FGDM_DPM_PLANE_M) return rec + "unknown plane " + std::to_string(src);
            if (src >= FGDM_DPM_PLANE_HIST0 && src < FGDM_DPM_PLANE_M && !written[src - FGDM_DPM_PLANE_HIST0])
                return rec + "reads history slot " + std::to_string(src - FGDM_DPM_PLANE_HIST0) + ", which no earlier record wrote";
        }
        if (p->slot[k] < -1 || p->slot[k] > 2) return rec + "slot " + std::to_string(p->slot[k]) + " is outside -1..2";
        if (p->dest[k] != FGDM_DPM_DEST_STATE && p->dest[k] != FGDM_DPM_DEST_EVAL) return rec + "unknown destination " + std::to_string(p->dest[k]);
        if (p->slot[k] >= 0) written[p->slot[k]] = true;
    }
    if (p->dest[p->n_eval - 1] != FGDM_DPM_DEST_STATE) return "the last record does not write the state";
    return "";
}

// DPM_Solver.sample (dpm_solver.py:965-1124) as a program: per record one evaluation of the network on the evaluation input, then
// one launch of k_dpm_program_step.  The evaluation input L.x2 is also the record's x_eval (io.x) (read and rewritten in place); the state
// x changes only behind a FGDM_DPM_DEST_STATE record, so the x at s survives the intermediate points of a singlestep update.
static int run_dpm_program(fgdm_engine* e, const fgdm_dpm_solver_params& p, hipStream_t s) {
    const int K = p.n_eval;
    const bool cfg_on = loop_cfg_on(p.uncond, p.cfg_scale);
    Loop L(e, s, p, K, cfg_on, loop_flags(p.flags, cfg_on));
    CHK(L.begin(p.cond, p.uncond, nullptr, p.t_float, 3));      // the model value of a record lives in plane slot[k]
    CHK(L.seed());
    float* const planes[4] = {L.x, L.plane(0), L.plane(1), L.plane(2)};
    int rc = FGDM_OK;
    for (int k = 0; k < K && rc == FGDM_OK; ++k) {
        rc = L.eval(k);
        if (rc != FGDM_OK) break;
        DpmProgramStep a{};
        rc = dpm_program_terms(a, planes, p.slot[k], p.nterms[k], p.plane + (size_t)k * DPM_MAX_TERMS, p.coef + (size_t)k * DPM_MAX_TERMS);
        if (rc != FGDM_OK) break;
        a.io = L.step_io(k, p.cfg_scale);
        a.io.x = L.x2;                  // x_eval; the state is the base plane
        if (p.dest[k] != FGDM_DPM_DEST_STATE) a.io.x_out = nullptr;
        a.conv_x = p.conv_x[k]; a.conv_e = p.conv_e[k];
        rc = dpm_program_step(a, s);
    }
    return rc;
}
int fgdm_sample_dpm_solver(fgdm_engine* e, const fgdm_dpm_solver_params* caller, void* stream) {
    return loop_entry(e, caller, stream, FGDM_DPM_SOLVER_PARAMS_SIZE_V1, "fgdm_sample_dpm_solver", "fgdm_dpm_solver_params", true,
                      [](const fgdm_dpm_solver_params& known) { return dpm_program_error(&known); }, run_dpm_program);
}

static const char* ancestral_params_error(const fgdm_ancestral_params* p, const fgdm_engine* e) {
    const bool armed = e->loop_noise.on;
    if (p->reserved0 != 0 || p->reserved1 != 0) return "reserved0 and reserved1 must be 0";
    if (!p->x || !p->cond || !p->timesteps || !p->sqrt_recip_alphas_cumprod || !p->sqrt_recipm1_alphas_cumprod ||
        !p->posterior_mean_coef1 || !p->posterior_mean_coef2 || !p->std)
        return "x, cond or a table is NULL";
    if (p->S <= 0 || p->B <= 0 || p->H <= 0 || p->W <= 0) return "S, B, H and W must be positive";
    if (p->mask && (!p->x0 || (!p->q_noise && !armed) || !p->sqrt_alphas_cumprod_t || !p->sqrt_one_minus_alphas_cumprod_t))
        return "mask needs x0, q_noise and q_sample's two coefficient tables";
    if (!p->step_noise && !armed)
        for (int i = 0; i < p->S; ++i)
            if (p->std[i] != 0.f) return "a std is not 0 and step_noise is NULL";
    if (armed)
        if (const char* why = loop_noise_range_error(e, p->B, p->S)) return why;
    return log_steps_error(p->log_steps, p->n_log, p->S);
}

// p_sample_loop (ddpm.py:1382-1430): per step one evaluation of the network on x, then one launch of k_ancestral_loop_step, which
// also does the step's own blend and writes x into the network's input.  Every table is in walk order.
static int run_ancestral(fgdm_engine* e, const fgdm_ancestral_params& p, hipStream_t s) {
    const int S = p.S;
    Loop L(e, s, p, S, false, loop_flags(p.flags, false), p.log_steps, p.n_log);
    CHK(L.begin(p.cond, nullptr, p.timesteps, nullptr, 0));
    CHK(L.seed());
    const size_t n = L.n;
    int rc = FGDM_OK;
    for (int i = 0; i < S && rc == FGDM_OK; ++i) {
        rc = L.eval(i);
        if (rc != FGDM_OK) break;
        AncestralLoopStep a{};
        a.io = L.step_io(i, 0.f);
        a.cr = p.sqrt_recip_alphas_cumprod[i]; a.crm1 = p.sqrt_recipm1_alphas_cumprod[i];
        a.c1 = p.posterior_mean_coef1[i]; a.c2 = p.posterior_mean_coef2[i]; a.std = p.std[i];
        a.noise = a.std != 0.f && p.step_noise ? p.step_noise + (size_t)i * n : nullptr;
        if (p.mask) {
            a.mask = p.mask; a.x0 = p.x0; a.qnoise = p.q_noise ? p.q_noise + (size_t)i * n : nullptr;
            a.sa_t = p.sqrt_alphas_cumprod_t[i]; a.s1m_t = p.sqrt_one_minus_alphas_cumprod_t[i];
        }
        a.gen = e->noise_gen(p.H, p.W, i, i, a.std != 0.f && !a.noise, a.mask && !a.qnoise);
        a.io.log_x = L.log_plane(p.x_inter_out, L.log_slot(i));
        rc = ancestral_loop_step(a, s);
    }
    return rc;
}
int fgdm_sample_ancestral(fgdm_engine* e, const fgdm_ancestral_params* caller, void* stream) {
    return loop_entry(e, caller, stream, FGDM_ANCESTRAL_PARAMS_SIZE_V1, "fgdm_sample_ancestral", "fgdm_ancestral_params", true,
                      [e](const fgdm_ancestral_params& known) { return ancestral_params_error(&known, e); }, run_ancestral);
}

static const char* ddim_encode_params_error(const fgdm_ddim_encode_params* p) {
    if (p->reserved0 != 0) return "reserved0 must be 0";
    if (!p->x || !p->cond || !p->timesteps || !p->cx || !p->ce) return "x, cond or a table is NULL";
    if (p->S <= 0 || p->B <= 0 || p->H <= 0 || p->W <= 0) return "S, B, H and W must be positive";
    return log_steps_error(p->log_steps, p->n_log, p->S);
}

// DDIMSampler.encode (ddim_hacked.py:234-279): per step one evaluation of the network on cat([x] * 2) (or x, CFG off), then one
// launch of k_invert_loop_step.
static int run_ddim_encode(fgdm_engine* e, const fgdm_ddim_encode_params& p, hipStream_t s) {
    const int S = p.S;
    const bool cfg_on = loop_cfg_on(p.uncond, p.cfg_scale);
    Loop L(e, s, p, S, cfg_on, loop_flags(p.flags, cfg_on), p.log_steps, p.n_log);
    CHK(L.begin(p.cond, p.uncond, p.timesteps, nullptr, 0));
    CHK(L.seed());
    int rc = FGDM_OK;
    for (int i = 0; i < S && rc == FGDM_OK; ++i) {
        rc = L.eval(i);
        if (rc != FGDM_OK) break;
        InvertLoopStep a{};
        a.io = L.step_io(i, p.cfg_scale);
        a.cx = p.cx[i]; a.ce = p.ce[i];
        a.io.log_x = L.log_plane(p.x_inter_out, L.log_slot(i));
        rc = invert_loop_step(a, s);
    }
    return rc;
}
int fgdm_ddim_encode(fgdm_engine* e, const fgdm_ddim_encode_params* caller, void* stream) {
    return loop_entry(e, caller, stream, FGDM_DDIM_ENCODE_PARAMS_SIZE_V1, "fgdm_ddim_encode", "fgdm_ddim_encode_params", true,
                      [](const fgdm_ddim_encode_params& known) { return ddim_encode_params_error(&known); }, run_ddim_encode);
}

}  // extern "C"
