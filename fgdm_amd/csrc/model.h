// Model description of the FG-DM engine: the networks as structs of (still empty) packed weights, the topology builders with
// their config checks, and ONE traversal per module kind that names every state-dict key, with its shape and the GemmW / NormW it
// lands in, exactly once.  Two visitors run that traversal: the Registrar below fills the parameter table (build()), the engine's
// Packer (engine.hip) uploads the kernel layouts (fgdm_finalize_weights).  A third, Units, wraps either kind of visitor and shows
// it only the packed layers a set of keys belongs to (fgdm_weights_*).  A traversal takes its references when it runs, so
// nothing here points into a Block or a Net that construction is still copying around.
//
// Reference structure being reproduced (file:line in the reference checkout):
//   UNetModel.__init__              ldm/modules/diffusionmodules/openaimodel.py:469-734
//   SpatialTransformer & friends    ldm/modules/attention.py:152-292
//   Adapter / TimeAdapter           ldm/modules/encoders/adapter.py:280-346, 387-417
//   ControlNet                      controlnet/cldm/cldm.py:545-813
//   Encoder / Decoder               ldm/modules/diffusionmodules/model.py:368-560
#pragma once
#include "engine_shared.h"

#include <cstdint>
#include <string>
#include <unordered_map>
#include <vector>

#define CHK0(x) do { int _rc0 = (x); if (_rc0 != FGDM_OK) return _rc0; } while (0)

namespace {

struct Tensor {
    half_t* p = nullptr;
    int B = 0, H = 0, W = 0, C = 0;
    size_t numel() const { return (size_t)B * H * W * C; }
    int rows() const { return B * H * W; }
};

struct ParamSlot {
    std::vector<int64_t> shape;
    std::vector<float> host;
    bool loaded = false;
    int comp = 0;           // index into Model::comps of the component (network) the key belongs to
    size_t numel() const { size_t n = 1; for (auto d : shape) n *= (size_t)d; return n; }
};

struct GemmW {              // packed [npad][K] fp16 weight + fp32 bias (packed column order)
    half_t* w = nullptr;
    float* bias = nullptr;
    int N = 0, K = 0;
    bool im2col = false;    // conv3x3 whose Cin is not a multiple of 64: K = roundup64(9 * cin_pad)
    int cin_pad = 0;
    int k_real = 0;         // un-padded contraction length (algorithmic flop accounting)
    half_t* wph = nullptr;  // Upsample convs of the UNets: the four 2x2 phase kernels [4][npad][4 Cin] next to the 3x3 pack (IG_CONV2_PHASE)
    float* ln_u = nullptr;  // LayerNorm folded in: u[n] = sum_k W'[n][k] (packed order); bias then holds sum_k beta_k W_nk + b_n
    float ln_eps = 1e-5f;
};
struct NormW { float* g = nullptr; float* b = nullptr; int C = 0; };

enum LType { L_CONV, L_RES, L_ATTN, L_DOWN, L_UP };
struct Layer {
    LType type = L_CONV;
    int cin = 0, cout = 0, heads = 0;
    bool down = false;                                     // L_RES with AvgPool2d(2) on both branches (TimeAdapter)
    std::string pre;
    GemmW conv;                                            // L_CONV / L_DOWN / L_UP
    NormW gn1, gn2; GemmW c1, c2, skip;                    // L_RES
    float eps = 1e-5f;                                     // L_RES GroupNorm eps: 1e-5 in the UNet, 1e-6 in the first stage
    int emb_off = -1;                                      // L_RES row offset in Net::emb_all; < 0: no timestep row (first stage)
    NormW gn, ln1, ln2, ln3;                               // L_ATTN
    GemmW pin, pout, qkv1, o1, q2, k2, v2, o2, ffp, ffo;     // qkv1: attn1's to_q | to_k | to_v stacked (one GEMM)
};
typedef std::vector<Layer> Block;

struct AdapterBlk { int ic = 0, oc = 0; bool down = false; std::string pre; GemmW in_conv, b1, b2; };

struct Net {
    std::string prefix;
    bool control = false;
    GemmW time0, time2, emb_all;
    int emb_total = 0;
    std::vector<Block> input, output;
    Block middle;
    NormW out_gn; GemmW out_conv;                          // UNet only
    bool has_adapter = false;                              // UNet only
    GemmW ad_conv_in; std::vector<AdapterBlk> ad_body;
    // AdaptUNetModel (openaimodel.py:993-999): num_prompts - 1 further Adapters over extra condition images; their
    // features do not depend on x or t, so their sum is computed once per set of conds (fgdm_set_adapter_conds)
    std::vector<GemmW> xad_conv_in; std::vector<std::vector<AdapterBlk>> xad_body;
    Tensor xad_sum[4]; bool xad_valid = false;
    bool time_adapter = false; Block tad_body;             // TimeAdapter: time-conditioned ResBlocks (adapter.py:387-417)
    std::vector<GemmW> zero_convs; GemmW mid_out;          // ControlNet only
    GemmW hint_convs[8];
    Tensor guided;                                         // cached input_hint_block output (persistent hipMalloc)
};

// f(block) for the input blocks, the middle block, the output blocks and -- with_tad -- the TimeAdapter's ResBlocks, in that
// order (the row order of Net::emb_all); stops at the first f that does not return FGDM_OK
template <class N, class F> int for_each_block(N& n, bool with_tad, F f) {
    for (auto& b : n.input) CHK0(f(b));
    CHK0(f(n.middle));
    for (auto& b : n.output) CHK0(f(b));
    return with_tad ? f(n.tad_body) : FGDM_OK;
}

// First-stage decoder (AutoencoderKL.decode; model.py:462-560).  Its ResnetBlocks (temb = None, model.py:121-141) are Layers of
// type L_RES without a timestep row.
struct VLevel { Block blocks; int ch = 0; bool up = false; std::string up_pre; GemmW upconv; };
struct VAttn { std::string pre; NormW norm; GemmW q, k, v, o; };      // AttnBlock (model.py:146-203)
// First-stage encoder (AutoencoderKL.encode; model.py:368-460), present when fgdm_config::vae_encoder is set
struct VDown { Block blocks; int ch = 0; bool down = false; std::string down_pre; GemmW downconv; };
struct VEnc {
    bool on = false;
    GemmW conv_in, conv_out;
    std::vector<VDown> levels;             // execution order: full resolution first
    Layer mid1, mid2;
    VAttn attn;
    NormW norm_out;
    float* qc = nullptr;                   // quant_conv: 64 weights [co][ci] + 8 biases
};
struct Vae {
    bool on = false;
    std::string prefix;
    int top = 0, factor = 1;
    GemmW conv_in, conv_out;
    Layer mid1, mid2;
    VAttn attn;
    std::vector<VLevel> levels;            // execution order: deepest level first
    NormW norm_out;
    float* pq = nullptr;                   // post_quant_conv: 16 weights [co][ci] + 4 biases
    VEnc enc;
};

// CLIP text encoder (transformers.CLIPTextModel behind FrozenCLIPEmbedder; ldm/modules/encoders/modules.py:137-162)
struct ClipLayer { std::string pre; NormW ln1, ln2; GemmW qkv, o, fc1, fc2; };
struct Clip {
    bool on = false;
    std::string prefix;
    float* tok = nullptr;     // [vocab][W] fp32 (nn.Embedding is not an autocast op: the residual stream starts in fp32)
    float* pos = nullptr;     // [max_len][W] fp32
    std::vector<ClipLayer> layers;
    NormW final_ln;
};

// One network of the engine, by state-dict prefix: it is (re)packed as a whole when tensors of it were loaded
struct Component { std::string prefix; bool dirty = false, packed = false; std::vector<void*> allocs; };

// What a Linear's packing needs beyond key and shape (the Registrar ignores it)
struct LinOpt {
    int q_head_dim = 0;     // > 0: a to_q projection (the first source of a stack): scaled by log2(e) d^-1/2
    bool geglu = false;     // ff.net.0.proj: value | gate rows interleaved in 64-row groups
    std::string ln;         // state-dict prefix of the LayerNorm whose output feeds this Linear (folded in unless FGDM_LN_FOLD=0)
};

// The keys of a ResBlock (openaimodel.py:203-257) and of the first stage's ResnetBlock (model.py:83-119): same modules, same order
struct ResKeys { const char *norm1, *conv1, *emb, *norm2, *conv2, *skip; };
const ResKeys UNET_RES{"in_layers.0", "in_layers.2", "emb_layers.1", "out_layers.0", "out_layers.3", "skip_connection"};
const ResKeys VAE_RES{"norm1", "conv1", nullptr, "norm2", "conv2", "nin_shortcut"};

const int ADAPTER_CH[4] = {320, 640, 1280, 1280};

struct Model {
    fgdm_config cfg{};
    std::string err;
    std::vector<std::string> order;
    std::unordered_map<std::string, ParamSlot> params;
    std::vector<Component> comps;        // the UNet, the ControlNets, the first stage, the text encoder
    int vae_comp = -1, clip_comp = -1;
    Net unet;
    std::vector<Net> cns;
    Vae vae;
    Clip clip;

    int fail(int code, const std::string& m) { err = m; return code; }

    // ------------------------------------------------------------------------------------ traversal: every key, once
    // A visitor `v` is told, in the reference's module-registration order:
    //   v.norm(NormW&, pre, C)  v.layernorm(NormW&, pre, C)  v.conv3(GemmW&, pre, cout, cin)  v.pointwise(float*&, pre, co, ci)
    //   v.linear(GemmW&, pre, N, K, conv1x1 shape, bias[, LinOpt])  v.table(float*&, key, rows, W)
    //   v.source(pre, N, K, bias): a Linear that exists only as a source of a stacked GEMM, and
    //   v.stack(GemmW&, {pre...}, bias[, LinOpt]): that GEMM, over sources declared before it.
    template <class V> void visit_res(V& v, Layer& l, const ResKeys& k, int temb = 0, std::vector<std::string>* embs = nullptr) {
        const std::string& p = l.pre;
        v.norm(l.gn1, p + k.norm1, l.cin);
        v.conv3(l.c1, p + k.conv1, l.cout, l.cin);
        if (k.emb) { v.source(p + k.emb, l.cout, temb, true); embs->push_back(p + k.emb); }      // packed into Net::emb_all
        v.norm(l.gn2, p + k.norm2, l.cout);
        v.conv3(l.c2, p + k.conv2, l.cout, l.cout);
        if (l.cin != l.cout) v.linear(l.skip, p + k.skip, l.cout, l.cin, /*conv1x1 shape*/ true, /*bias*/ true);
    }
    template <class V> void visit_attn(V& v, Layer& l) {
        const std::string& p = l.pre;
        const std::string t = p + "transformer_blocks.0.";
        const std::string q = t + "attn1.to_q", k = t + "attn1.to_k", vv = t + "attn1.to_v", n1 = t + "norm1", n2 = t + "norm2", n3 = t + "norm3";
        const int ch = l.cin, d = ch / l.heads;
        v.norm(l.gn, p + "norm", ch);
        const bool conv_proj = !cfg.use_linear_in_transformer;      // nn.Conv2d(C, C, 1) or nn.Linear(C, C): the same GEMM over NHWC rows
        v.linear(l.pin, p + "proj_in", ch, ch, conv_proj, true);
        v.source(q, ch, ch, false);
        v.source(k, ch, ch, false);
        v.source(vv, ch, ch, false);
        v.stack(l.qkv1, {q, k, vv}, false, LinOpt{d, false, n1});
        v.linear(l.o1, t + "attn1.to_out.0", ch, ch, false, true);
        v.linear(l.ffp, t + "ff.net.0.proj", 8 * ch, ch, false, true, LinOpt{0, true, n3});
        v.linear(l.ffo, t + "ff.net.2", ch, 4 * ch, false, true);
        v.linear(l.q2, t + "attn2.to_q", ch, ch, false, false, LinOpt{d, false, n2});
        v.linear(l.k2, t + "attn2.to_k", ch, cfg.context_dim, false, false);
        v.linear(l.v2, t + "attn2.to_v", ch, cfg.context_dim, false, false);
        v.linear(l.o2, t + "attn2.to_out.0", ch, ch, false, true);
        v.layernorm(l.ln1, n1, ch);
        v.layernorm(l.ln2, n2, ch);
        v.layernorm(l.ln3, n3, ch);
        v.linear(l.pout, p + "proj_out", ch, ch, conv_proj, true);
    }
    template <class V> void visit_block(V& v, Block& blk, int temb, std::vector<std::string>* embs) {
        for (Layer& l : blk)
            switch (l.type) {
                case L_CONV: v.conv3(l.conv, l.pre.substr(0, l.pre.size() - 1), l.cout, l.cin); break;
                case L_RES: visit_res(v, l, UNET_RES, temb, embs); break;
                case L_ATTN: visit_attn(v, l); break;
                case L_DOWN: v.conv3(l.conv, l.pre + "op", l.cin, l.cin); break;
                case L_UP: v.conv3_up(l.conv, l.pre + "conv", l.cin, l.cin); break;
            }
    }
    // Adapter (adapter.py:280-332): the 8 ResnetBlocks (or, TimeAdapter, `tad` ResBlocks), then conv_in
    template <class V> void visit_adapter(V& v, GemmW& conv_in, std::vector<AdapterBlk>& body, const std::string& ap, Block* tad = nullptr,
                                          int temb = 0, std::vector<std::string>* embs = nullptr) {
        if (tad) visit_block(v, *tad, temb, embs);
        for (AdapterBlk& b : body) {
            if (b.ic != b.oc) v.linear(b.in_conv, b.pre + "in_conv", b.oc, b.ic, true, true);
            v.conv3(b.b1, b.pre + "block1", b.oc, b.oc);
            v.linear(b.b2, b.pre + "block2", b.oc, b.oc, true, true);
        }
        v.conv3(conv_in, ap + "conv_in", ADAPTER_CH[0], cfg.in_channels);
    }
    // UNetModel (openaimodel.py:537-728) / ControlNet (cldm.py:640-787)
    template <class V> void visit_net(V& v, Net& n) {
        const std::string& p = n.prefix;
        const int mc = cfg.model_channels, temb = 4 * mc, ch = n.middle.back().cout;
        std::vector<std::string> embs, tad_embs;
        v.linear(n.time0, p + "time_embed.0", temb, mc, false, true);
        v.linear(n.time2, p + "time_embed.2", temb, temb, false, true);
        if (n.has_adapter) {         // the adapter precedes input_blocks (openaimodel.py:551-558)
            visit_adapter(v, n.ad_conv_in, n.ad_body, p + "adapter.", n.time_adapter ? &n.tad_body : nullptr, temb, &tad_embs);
            for (size_t kk = 0; kk < n.xad_body.size(); ++kk) visit_adapter(v, n.xad_conv_in[kk], n.xad_body[kk], p + "adapters." + std::to_string(kk) + ".");
        }
        for (Block& b : n.input) visit_block(v, b, temb, &embs);
        if (n.control) {
            for (size_t i = 0; i < n.input.size(); ++i) {
                const int zc = n.input[i].back().type == L_DOWN ? n.input[i].back().cin : n.input[i][0].cout;
                v.linear(n.zero_convs[i], p + "zero_convs." + std::to_string(i) + ".0", zc, zc, true, true);
            }
            static const int hc[7] = {16, 16, 32, 32, 96, 96, 256};
            int prev = cfg.hint_channels;
            for (int k = 0; k < 8; ++k) {
                const int oc = k < 7 ? hc[k] : mc;
                v.conv3(n.hint_convs[k], p + "input_hint_block." + std::to_string(2 * k), oc, prev);
                prev = oc;
            }
        }
        visit_block(v, n.middle, temb, &embs);
        if (n.control) {
            v.linear(n.mid_out, p + "middle_block_out.0", ch, ch, true, true);
        } else {
            for (Block& b : n.output) visit_block(v, b, temb, &embs);
            v.norm(n.out_gn, p + "out.0", mc);
            v.conv3(n.out_conv, p + "out.2", cfg.out_channels, mc);
        }
        // every ResBlock's emb_layers Linear stacked into one GEMM per evaluation (openaimodel.py:238-244, 290), rows in
        // for_each_block's order: Layer::emb_off
        embs.insert(embs.end(), tad_embs.begin(), tad_embs.end());
        v.stack(n.emb_all, embs, true);
    }
    template <class V> void visit_vattn(V& v, VAttn& at, int c) {
        v.norm(at.norm, at.pre + "norm", c);
        v.linear(at.q, at.pre + "q", c, c, true, true);
        v.linear(at.k, at.pre + "k", c, c, true, true);
        v.linear(at.v, at.pre + "v", c, c, true, true);
        v.linear(at.o, at.pre + "proj_out", c, c, true, true);
    }
    template <class V> void visit_vmid(V& v, Layer& mid1, VAttn& attn, Layer& mid2) {
        visit_res(v, mid1, VAE_RES);
        visit_vattn(v, attn, mid1.cout);
        visit_res(v, mid2, VAE_RES);
    }
    // AutoencoderKL (autoencoder.py:298-303): encoder.*, decoder.*, quant_conv.*, post_quant_conv.*
    template <class V> void visit_vae(V& v) {
        const int zc2 = 2 * cfg.vae_z_channels;
        if (vae.enc.on) {            // Encoder.__init__ (model.py:368-435) with double_z = True and in_channels = 3
            VEnc& en = vae.enc;
            const std::string d = vae.prefix + "encoder.";
            v.conv3(en.conv_in, d + "conv_in", cfg.vae_ch, 3);          // Cin = 3: the im2col layout, cin_pad 4
            for (VDown& lv : en.levels) {
                for (Layer& r : lv.blocks) visit_res(v, r, VAE_RES);
                if (lv.down) v.conv3(lv.downconv, lv.down_pre, lv.ch, lv.ch);
            }
            visit_vmid(v, en.mid1, en.attn, en.mid2);
            v.norm(en.norm_out, d + "norm_out", en.mid2.cout);
            v.conv3(en.conv_out, d + "conv_out", zc2, en.mid2.cout);
        }
        const std::string d = vae.prefix + "decoder.";      // Decoder.__init__ (model.py:486-530)
        v.conv3(vae.conv_in, d + "conv_in", vae.top, 4);
        visit_vmid(v, vae.mid1, vae.attn, vae.mid2);
        for (size_t i = vae.levels.size(); i-- > 0;) {      // `self.up.insert(0, up)`: registered ascending, run descending
            VLevel& lv = vae.levels[i];
            for (Layer& r : lv.blocks) visit_res(v, r, VAE_RES);
            if (lv.up) v.conv3(lv.upconv, lv.up_pre, lv.ch, lv.ch);
        }
        v.norm(vae.norm_out, d + "norm_out", vae.levels.back().ch);
        v.conv3(vae.conv_out, d + "conv_out", cfg.vae_out_ch, vae.levels.back().ch);
        if (vae.enc.on) v.pointwise(vae.enc.qc, vae.prefix + "quant_conv", zc2, zc2);
        v.pointwise(vae.pq, vae.prefix + "post_quant_conv", 4, 4);
    }
    // CLIPTextModel
    template <class V> void visit_clip(V& v) {
        const int W = cfg.clip_width, I = cfg.clip_mlp;
        v.table(clip.tok, clip.prefix + "embeddings.token_embedding.weight", cfg.clip_vocab, W);
        v.table(clip.pos, clip.prefix + "embeddings.position_embedding.weight", cfg.clip_max_len, W);
        for (ClipLayer& l : clip.layers) {
            const std::string a = l.pre + "self_attn.", q = a + "q_proj", k = a + "k_proj", vv = a + "v_proj";
            v.source(k, W, W, true);
            v.source(vv, W, W, true);
            v.source(q, W, W, true);
            v.stack(l.qkv, {q, k, vv}, true);
            v.linear(l.o, a + "out_proj", W, W, false, true);
            v.norm(l.ln1, l.pre + "layer_norm1", W);
            v.linear(l.fc1, l.pre + "mlp.fc1", I, W, false, true);
            v.linear(l.fc2, l.pre + "mlp.fc2", W, I, false, true);
            v.norm(l.ln2, l.pre + "layer_norm2", W);
        }
        v.norm(clip.final_ln, clip.prefix + "final_layer_norm", W);
    }
    template <class V> void visit_component(int c, V& v) {
        if (c == 0) visit_net(v, unet);
        else if (c <= (int)cns.size()) visit_net(v, cns[c - 1]);
        else if (c == vae_comp) visit_vae(v);
        else visit_clip(v);
    }

    // The registrar: key and shape into the parameter table, the slot tagged with its component
    struct Registrar {
        Model& m;
        int comp;
        void reg(const std::string& name, std::vector<int64_t> shape) {
            m.order.push_back(name);
            ParamSlot& ps = m.params[name];
            ps.shape = std::move(shape);
            ps.comp = comp;
        }
        void wb(const std::string& pre, std::vector<int64_t> wshape, bool bias = true) {
            const int64_t n = wshape[0];
            reg(pre + ".weight", std::move(wshape));
            if (bias) reg(pre + ".bias", {n});
        }
        void norm(NormW&, const std::string& pre, int C) { wb(pre, {C}); }
        void layernorm(NormW&, const std::string& pre, int C) { wb(pre, {C}); }
        void conv3(GemmW&, const std::string& pre, int cout, int cin) { wb(pre, {cout, cin, 3, 3}); }
        void conv3_up(GemmW& g, const std::string& pre, int cout, int cin) { conv3(g, pre, cout, cin); }
        void pointwise(float*&, const std::string& pre, int co, int ci) { wb(pre, {co, ci, 1, 1}); }
        void table(float*&, const std::string& key, int rows, int W) { reg(key, {rows, W}); }
        void source(const std::string& pre, int N, int K, bool bias) { wb(pre, {N, K}, bias); }
        void linear(GemmW&, const std::string& pre, int N, int K, bool conv1x1, bool bias, const LinOpt& = LinOpt()) {
            if (conv1x1) wb(pre, {N, K, 1, 1}, bias); else wb(pre, {N, K}, bias);
        }
        void stack(GemmW&, const std::vector<std::string>&, bool, const LinOpt& = LinOpt()) {}
    };

    // The third use of the traversal: the PACKED UNITS.  Every visitor call that packs something -- one GemmW, NormW or table -- is
    // one unit, built from the state-dict keys listed here: a Linear's weight and bias, the LayerNorm folded into it (ln_fold: the
    // engine's FGDM_LN_FOLD), every source of a stacked GEMM.  f(keys, replay) is told each unit; replay(visitor) repeats the call on
    // another visitor, so the engine re-packs (its Packer) or collects the buffers of exactly the units it picks.
    typedef std::vector<std::string> Keys;
    template <class F> struct Units {
        bool ln_fold;
        F f;
        static Keys wb(Keys k, const std::string& pre, bool bias = true) {
            k.push_back(pre + ".weight");
            if (bias) k.push_back(pre + ".bias");
            return k;
        }
        Keys folded(Keys k, const LinOpt& o) const { return ln_fold && !o.ln.empty() ? wb(std::move(k), o.ln) : k; }
        void norm(NormW& n, const std::string& pre, int C) { f(wb({}, pre), [&](auto& v) { v.norm(n, pre, C); }); }
        void layernorm(NormW& n, const std::string& pre, int C) { if (!ln_fold) f(wb({}, pre), [&](auto& v) { v.layernorm(n, pre, C); }); }
        void conv3(GemmW& g, const std::string& pre, int co, int ci) { f(wb({}, pre), [&](auto& v) { v.conv3(g, pre, co, ci); }); }
        void conv3_up(GemmW& g, const std::string& pre, int co, int ci) { f(wb({}, pre), [&](auto& v) { v.conv3_up(g, pre, co, ci); }); }
        void pointwise(float*& d, const std::string& pre, int co, int ci) { f(wb({}, pre), [&](auto& v) { v.pointwise(d, pre, co, ci); }); }
        void table(float*& d, const std::string& key, int rows, int W) { f(Keys{key}, [&](auto& v) { v.table(d, key, rows, W); }); }
        void source(const std::string&, int, int, bool) {}
        void linear(GemmW& g, const std::string& pre, int N, int K, bool c1, bool bias, const LinOpt& o = LinOpt()) {
            f(folded(wb({}, pre, bias), o), [&](auto& v) { v.linear(g, pre, N, K, c1, bias, o); });
        }
        void stack(GemmW& g, const std::vector<std::string>& pres, bool bias, const LinOpt& o = LinOpt()) {
            Keys k;
            for (auto& pre : pres) k = wb(std::move(k), pre, bias);
            f(folded(std::move(k), o), [&](auto& v) { v.stack(g, pres, bias, o); });
        }
    };
    template <class F> void visit_units(bool ln_fold, F f) {
        Units<F> u{ln_fold, f};
        for (int c = 0; c < (int)comps.size(); ++c) visit_component(c, u);
    }
    // the key sets of the units that own any of `touched` (pure: no device), in traversal order
    template <class Has> std::vector<Keys> plan_units(bool ln_fold, Has touched) {
        std::vector<Keys> out;
        visit_units(ln_fold, [&](const Keys& keys, auto&&) {
            for (auto& k : keys) if (touched(k)) { out.push_back(keys); break; }
        });
        return out;
    }

    // ------------------------------------------------------------------------------------ topology: which layers, what channels
    static Layer mk(LType t, int cin, int cout, int heads = 0) {
        Layer l; l.type = t; l.cin = cin; l.cout = cout; l.heads = heads; return l;
    }
    bool in_ares(int ds) const {
        for (int i = 0; i < cfg.n_attention_resolutions; ++i) if (cfg.attention_resolutions[i] == ds) return true;
        return false;
    }
    // The body of Adapter / TimeAdapter(cin, [320,640,1280,1280], nums_rb=2, use_conv=False) (openaimodel.py:554): 8 blocks under
    // `ap`body.K., the first of levels 1..3 downsampling; add(ic, oc, down, prefix) makes one
    template <class Add> static void adapter_body(const std::string& ap, Add add) {
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 2; ++j) {
                const bool down = (i != 0 && j == 0);
                add(down ? ADAPTER_CH[i - 1] : ADAPTER_CH[i], ADAPTER_CH[i], down, ap + "body." + std::to_string(i * 2 + j) + ".");
            }
    }
    static void name_layers(Block& blk, const std::string& pre) {
        for (size_t j = 0; j < blk.size(); ++j) blk[j].pre = pre + std::to_string(j) + ".";
    }
    // openaimodel.py:558-718 / cldm.py:640-787
    void build_net(Net& n, const std::string& prefix, bool control, int adapter_kind) {
        n.prefix = prefix; n.control = control; n.has_adapter = adapter_kind != 0; n.time_adapter = adapter_kind == 2;
        const int mc = cfg.model_channels;
        // heads of a SpatialTransformer at `c` channels: c / num_head_channels when the head WIDTH is fixed (openaimodel.py:603-606,
        // 659-662, 709-712), else num_heads at every level
        auto heads_at = [&](int c) { return cfg.num_head_channels > 0 ? c / cfg.num_head_channels : cfg.num_heads; };
        auto blocks = [](const std::string& ap) {
            std::vector<AdapterBlk> body;
            adapter_body(ap, [&](int ic, int oc, bool down, const std::string& pre) {
                AdapterBlk b; b.ic = ic; b.oc = oc; b.down = down; b.pre = pre; body.push_back(b); });
            return body;
        };
        if (adapter_kind == 1) {
            n.ad_body = blocks(prefix + "adapter.");
            const int nx = control ? 0 : cfg.n_extra_adapters;
            n.xad_conv_in.resize(nx);
            for (int kk = 0; kk < nx; ++kk) n.xad_body.push_back(blocks(prefix + "adapters." + std::to_string(kk) + "."));
        }
        if (n.time_adapter)
            adapter_body(prefix + "adapter.", [&](int ic, int oc, bool down, const std::string& pre) {
                Layer l = mk(L_RES, ic, oc); l.down = down; l.pre = pre; n.tad_body.push_back(l); });
        std::vector<int> chans;
        int ch = mc, ds = 1;
        n.input.push_back({mk(L_CONV, cfg.in_channels, mc)});
        chans.push_back(mc);
        for (int level = 0; level < cfg.n_levels; ++level) {
            const int mult = cfg.channel_mult[level];
            for (int r = 0; r < cfg.num_res_blocks; ++r) {
                Block b{mk(L_RES, ch, mult * mc)};
                ch = mult * mc;
                if (in_ares(ds)) b.push_back(mk(L_ATTN, ch, ch, heads_at(ch)));
                n.input.push_back(b);
                chans.push_back(ch);
            }
            if (level != cfg.n_levels - 1) {
                n.input.push_back({mk(L_DOWN, ch, ch)});
                chans.push_back(ch);
                ds *= 2;
            }
        }
        n.middle = {mk(L_RES, ch, ch), mk(L_ATTN, ch, ch, heads_at(ch)), mk(L_RES, ch, ch)};
        if (control) n.zero_convs.resize(n.input.size());
        for (int level = cfg.n_levels - 1; level >= 0 && !control; --level) {
            const int mult = cfg.channel_mult[level];
            for (int i = 0; i <= cfg.num_res_blocks; ++i) {
                const int ich = chans.back();
                chans.pop_back();
                Block b{mk(L_RES, ch + ich, mc * mult)};
                ch = mc * mult;
                if (in_ares(ds)) b.push_back(mk(L_ATTN, ch, ch, heads_at(ch)));
                if (level && i == cfg.num_res_blocks) { b.push_back(mk(L_UP, ch, ch)); ds /= 2; }
                n.output.push_back(b);
            }
        }
        // the containers have their final size: names, and every ResBlock's rows in emb_all
        for (size_t i = 0; i < n.input.size(); ++i) name_layers(n.input[i], prefix + "input_blocks." + std::to_string(i) + ".");
        name_layers(n.middle, prefix + "middle_block.");
        for (size_t i = 0; i < n.output.size(); ++i) name_layers(n.output[i], prefix + "output_blocks." + std::to_string(i) + ".");
        for_each_block(n, true, [&](Block& b) {
            for (Layer& l : b) if (l.type == L_RES) { l.emb_off = n.emb_total; n.emb_total += l.cout; }
            return FGDM_OK;
        });
    }
    static Layer vres(const std::string& pre, int cin, int cout) {
        Layer l = mk(L_RES, cin, cout); l.pre = pre; l.eps = 1e-6f; return l;      // Normalize = GroupNorm(32, eps 1e-6)
    }
    static void build_vmid(const std::string& d, int c, Layer& mid1, VAttn& attn, Layer& mid2) {
        mid1 = vres(d + "mid.block_1.", c, c);
        attn.pre = d + "mid.attn_1.";
        mid2 = vres(d + "mid.block_2.", c, c);
    }
    int build_vae() {
        const int L = cfg.vae_n_levels, ch = cfg.vae_ch, nrb = cfg.vae_num_res_blocks;
        if (L < 1 || L > FGDM_MAX_LEVELS || (ch & 63) || nrb < 0 || cfg.vae_z_channels != 4 || cfg.vae_out_ch < 1 || cfg.vae_out_ch > 8)
            return fail(FGDM_ERR_ARG, "unsupported first-stage decoder config (ch multiple of 64, z_channels 4, no attention at up levels)");
        Vae& v = vae;
        v.on = true;
        v.prefix = "first_stage_model.";
        v.factor = 1 << (L - 1);
        v.top = ch * cfg.vae_ch_mult[L - 1];
        if (cfg.vae_encoder) {
            VEnc& en = v.enc;
            en.on = true;
            const std::string d = v.prefix + "encoder.";
            int block_in = ch;
            en.levels.resize(L);
            for (int lvl = 0; lvl < L; ++lvl) {
                const std::string lp = d + "down." + std::to_string(lvl) + ".";
                VDown& lv = en.levels[lvl];
                for (int i = 0; i < nrb; ++i) { lv.blocks.push_back(vres(lp + "block." + std::to_string(i) + ".", block_in, ch * cfg.vae_ch_mult[lvl])); block_in = lv.blocks.back().cout; }
                lv.ch = block_in;
                lv.down = lvl != L - 1;
                lv.down_pre = lp + "downsample.conv";
            }
            build_vmid(d, block_in, en.mid1, en.attn, en.mid2);
        }
        const std::string d = v.prefix + "decoder.";
        build_vmid(d, v.top, v.mid1, v.attn, v.mid2);
        int block_in = v.top;
        for (int lvl = L - 1; lvl >= 0; --lvl) {      // execution order (model.py:501-511)
            const std::string lp = d + "up." + std::to_string(lvl) + ".";
            VLevel lv;
            lv.ch = ch * cfg.vae_ch_mult[lvl];
            for (int i = 0; i <= nrb; ++i) { lv.blocks.push_back(vres(lp + "block." + std::to_string(i) + ".", block_in, lv.ch)); block_in = lv.ch; }
            lv.up = lvl != 0;
            lv.up_pre = lp + "upsample.conv";
            v.levels.push_back(lv);
        }
        return FGDM_OK;
    }
    int build_clip() {
        const int W = cfg.clip_width, I = cfg.clip_mlp;
        if (cfg.clip_layers > 64 || (W & 63) || (I & 63) || cfg.clip_heads <= 0 || W != 64 * cfg.clip_heads ||
            cfg.clip_vocab <= 0 || cfg.clip_max_len <= 0 || cfg.clip_max_len > 128)
            return fail(FGDM_ERR_ARG, "unsupported text-encoder config (head dim must be 64, width/mlp multiples of 64, <= 128 tokens)");
        clip.on = true;
        clip.prefix = "cond_stage_model.transformer.text_model.";      // the reference checkpoints' prefix
        clip.layers.resize(cfg.clip_layers);
        for (int i = 0; i < cfg.clip_layers; ++i) clip.layers[i].pre = clip.prefix + "encoder.layers." + std::to_string(i) + ".";
        return FGDM_OK;
    }
    int add_component(const std::string& prefix) {
        comps.push_back(Component{prefix});
        return (int)comps.size() - 1;
    }
    int build() {
        if (cfg.n_levels < 1 || cfg.n_levels > FGDM_MAX_LEVELS || cfg.model_channels <= 0 || (cfg.model_channels & 63) ||
            cfg.n_controlnets < 0 || cfg.n_controlnets > FGDM_MAX_CONTROLNETS ||
            (cfg.context_dim & 63) || cfg.in_channels < 4 || cfg.in_channels > 32)
            return fail(FGDM_ERR_ARG, "unsupported config (model_channels and context_dim must be multiples of 64, 4 <= in_channels <= 32)");
        // in_channels > 4: the UNet reads cat([x] + c_concat, 1) (DiffusionWrapper 'hybrid', ddpm.py:1838-1841)
        if (cfg.in_channels != 4 && cfg.use_adapter)
            return fail(FGDM_ERR_ARG, "in_channels != 4 with use_adapter: UNetModel.forward hands the concatenated input to an adapter built "
                                      "for 4 channels (openaimodel.py:836-844); build the plain UNet (use_adapter = 0)");
        if (cfg.in_channels != 4 && cfg.n_controlnets > 0)
            return fail(FGDM_ERR_ARG, "in_channels != 4 with ControlNets: ControlLDM.apply_model never goes through DiffusionWrapper, its "
                                      "c_concat is the hint (cldm.py:836-849)");
        // num_heads XOR num_head_channels (openaimodel.py:507-511); -1, the reference's "unset", and 0, a zeroed struct, both mean unset
        const bool fixed_width = cfg.num_head_channels > 0, fixed_count = cfg.num_heads > 0;
        if (cfg.reserved0 != 0) return fail(FGDM_ERR_ARG, "fgdm_config::reserved0 must be 0");
        if (fixed_width == fixed_count)
            return fail(FGDM_ERR_ARG, fixed_width ? "num_heads and num_head_channels are both set: set one, leave the other -1"
                                                  : "either num_heads or num_head_channels has to be set");
        if (cfg.num_head_channels < -1 || cfg.num_heads < -1 || (fixed_width && (cfg.num_head_channels & 7)))
            return fail(FGDM_ERR_ARG, "num_head_channels must be a positive multiple of 8 (or -1), num_heads positive (or -1)");
        if (cfg.use_linear_in_transformer < 0 || cfg.use_linear_in_transformer > 1)
            return fail(FGDM_ERR_ARG, "use_linear_in_transformer: 0 (1x1 convolutions) or 1 (nn.Linear proj_in / proj_out)");
        for (int l = 0; l < cfg.n_levels; ++l) {
            const int ch = cfg.model_channels * cfg.channel_mult[l];
            if (fixed_width ? ch % cfg.num_head_channels : ch % cfg.num_heads)
                return fail(FGDM_ERR_ARG, fixed_width ? "channels not divisible by num_head_channels" : "channels not divisible by heads");
        }
        if (cfg.use_adapter && !(cfg.model_channels == 320 && cfg.n_levels == 4 && cfg.num_res_blocks == 2))
            return fail(FGDM_ERR_ARG, "FG-DM adapter requires the SD-v1 topology (openaimodel.py:554-556,855-859)");
        if (cfg.use_adapter < 0 || cfg.use_adapter > 2) return fail(FGDM_ERR_ARG, "use_adapter: 0 none, 1 Adapter, 2 TimeAdapter");
        if (cfg.n_extra_adapters < 0 || cfg.n_extra_adapters > 7 || (cfg.n_extra_adapters && cfg.use_adapter != 1))
            return fail(FGDM_ERR_ARG, "n_extra_adapters (AdaptUNetModel num_prompts - 1) needs use_adapter = 1");
        build_net(unet, "model.diffusion_model.", false, cfg.use_adapter);
        add_component(unet.prefix);
        cns.resize(cfg.n_controlnets);
        for (int k = 0; k < cfg.n_controlnets; ++k) {
            build_net(cns[k], k == 0 ? std::string("control_model.") : "control_model_" + std::to_string(k) + ".", true, 0);
            add_component(cns[k].prefix);
        }
        if (cfg.vae_encoder < 0 || cfg.vae_encoder > 1 || (cfg.vae_encoder && cfg.vae_ch <= 0))
            return fail(FGDM_ERR_ARG, "vae_encoder: 0 none, 1 first-stage encoder (needs the first-stage config: vae_ch > 0)");
        if (cfg.vae_ch > 0) { CHK0(build_vae()); vae_comp = add_component(vae.prefix); }
        if (cfg.clip_layers > 0) { CHK0(build_clip()); clip_comp = add_component(clip.prefix); }
        for (int c = 0; c < (int)comps.size(); ++c) { Registrar r{*this, c}; visit_component(c, r); }
        return FGDM_OK;
    }
};

}  // namespace
