/* libfgdm_hip.so -- C ABI of the MI355X-native FG-DM sampling engine.
 *
 * Drop-in boundary for the hot path named in BASELINE.json.  Each entry point states the
 * reference interface it replaces (paths relative to the DeepakSridhar/fgdm checkout).  Conventions:
 *   - return 0 on success, negative FGDM_ERR_* otherwise; nothing throws across the ABI;
 *     fgdm_last_error() gives a message for the last failing call on that engine;
 *   - all tensor arguments are DEVICE pointers owned by the caller (e.g. torch tensor.data_ptr()), except
 *     fgdm_load_tensor which accepts host or device memory;
 *   - latents / eps are fp32 NCHW [B,4,H,W] (also for in_channels > 4: the further input channels come from the tensor registered
 *     with the concat entry below, never through x); timesteps int64 [B]; context fp32 [B,77,ctx_dim] ("77" below: the engine's
 *     context token count, 77 unless fgdm_set_context_tokens changed it);
 *     hints fp32 NCHW [B,3,8H,8W] in [0,1];
 *   - the engine owns weights and workspace; one engine per device; not thread-safe; all work is enqueued on
 *     the stream passed in (a hipStream_t cast to void*; NULL = default stream), no implicit synchronisation.
 */
#ifndef FGDM_H
#define FGDM_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define FGDM_MAX_LEVELS 8
#define FGDM_MAX_CONTROLNETS 4

typedef struct fgdm_engine fgdm_engine;

/* Hyper-parameters of UNetModel / ControlNet: the keys of models/config.yaml:33-48 and
 * controlnet/models/cldm_v15_canny.yaml:21-53 (use_spatial_transformer=True, transformer_depth=1, legacy=False). */
typedef struct fgdm_config {
    int32_t in_channels, out_channels, model_channels, num_res_blocks;
    int32_t n_levels;
    int32_t channel_mult[FGDM_MAX_LEVELS];
    int32_t n_attention_resolutions;
    int32_t attention_resolutions[FGDM_MAX_LEVELS];
    int32_t num_heads, context_dim;
    int32_t use_adapter;       /* FG-DM self-prompt adapter (openaimodel.py:551-556): 0 none (no_prompting), 1 Adapter,
                                * 2 TimeAdapter (use_time_adapter=True; ldm/modules/encoders/adapter.py:387-417) */
    int32_t n_controlnets;     /* 0..FGDM_MAX_CONTROLNETS ControlNet twin encoders (cldm.py:545-790) */
    int32_t hint_channels;     /* 3 */
    int64_t workspace_bytes;   /* initial activation slab; 0 = default; grows on demand */
    /* First-stage decoder (AutoencoderKL ddconfig, models/config.yaml:55-69); vae_ch = 0: engine without a decoder */
    int32_t vae_ch, vae_n_levels;
    int32_t vae_ch_mult[FGDM_MAX_LEVELS];
    int32_t vae_num_res_blocks, vae_z_channels, vae_out_ch;
    /* Text encoder (transformers.CLIPTextModel behind FrozenCLIPEmbedder, ldm/modules/encoders/modules.py:137-162);
     * clip_layers = 0: engine without one.  openai/clip-vit-large-patch14: 12 layers, width 768, 12 heads, mlp 3072,
     * vocab 49408, 77 positions. */
    int32_t clip_layers, clip_width, clip_heads, clip_mlp, clip_vocab, clip_max_len;
    int32_t n_extra_adapters;  /* AdaptUNetModel num_prompts - 1 (openaimodel.py:993-999): further Adapters whose features are
                                * summed onto the FG-DM adapter's; needs use_adapter = 1 */
    int32_t vae_encoder;       /* 0: first-stage DECODER only (the parameter table ends decoder.*, post_quant_conv.*); 1: the whole
                                * AutoencoderKL in its registration order (ldm/models/autoencoder.py:298-303): encoder.*, decoder.*,
                                * quant_conv.*, post_quant_conv.*, with double_z = True and in_channels = 3 (models/config.yaml:55-69)
                                * and the ch / ch_mult / num_res_blocks / z_channels above.  Needs vae_ch > 0.  (Appended last: the
                                * offsets of the earlier fields are those of engines built before the encoder existed.) */
    int32_t reserved0;         /* must be 0.  Offset 204: the tail padding of the 208-byte struct that ended with vae_encoder, so
                                * the fields below start where that struct ended and none of its bytes changes meaning. */
    /* The second Stable-Diffusion family (SD-2.x UNets and their ControlNets; UNetModel.__init__, openaimodel.py:469-734).  Both
     * fields zero (or -1 / 0): the networks above, unchanged.
     * num_head_channels > 0: every SpatialTransformer at `ch` channels has ch / num_head_channels heads of that width (64 in
     *   SD-2.x: 5 / 10 / 20 / 20 heads) and num_heads must be -1 or 0; a multiple of 8 that divides every level's channel count,
     *   and a width the attention kernels are built for (40, 64, 80, 160).  0 or -1: num_heads heads at every level.
     * use_linear_in_transformer = 1: SpatialTransformer.proj_in / proj_out are nn.Linear, so their weights are [C, C] in the
     *   parameter table instead of [C, C, 1, 1] (ldm/modules/attention.py:262-267,285-291).  The arithmetic is the same GEMM. */
    int32_t num_head_channels;
    int32_t use_linear_in_transformer;
} fgdm_config;

#define FGDM_DTYPE_F32 0
#define FGDM_DTYPE_F16 1

/* flags for fgdm_apply_model */
#define FGDM_FLAG_USE_ORIGINAL 1      /* UNetModel.forward_original: skip the adapter (openaimodel.py:818-822) */
#define FGDM_FLAG_ONLY_MID_CONTROL 2  /* ControlledUnetModel only_mid_control (cldm.py:43-44) */
#define FGDM_FLAG_NO_CONTROL 4        /* cond['c_concat'] is None branch (cldm.py:842-843) */
#define FGDM_FLAG_CFG_PAIRS 8         /* the batch is cat([x]*2), cat([t]*2) of a classifier-free-guidance step (ddim.py:222-
                                       * 226; same pcond, and the cached hint covers B/2 rows): rows b and b + B/2 differ only
                                       * in the context, so the network up to its first cross-attention runs once on B/2 rows.
                                       * Results are bit-identical to the call without the flag.  The flag is the CALLER's
                                       * assertion that the halves are equal: with it only rows [0, B/2) of x, t and pcond are
                                       * read for that prefix (pcond must still hold B rows); the host mirrors verify pcond
                                       * before setting it (fgdm_amd/models.py). */

int fgdm_create(const fgdm_config* cfg, int device, fgdm_engine** out);
void fgdm_destroy(fgdm_engine* e);
const char* fgdm_last_error(const fgdm_engine* e);   /* e == NULL: why the last fgdm_create failed */

/* Parameter table: the reference state_dict keys the engine expects.  UNet keys carry the prefix
 * "model.diffusion_model." (adapter: "model.diffusion_model.adapter."), ControlNet k uses "control_model."
 * (k = 0) or "control_model_<k>." -- the names load_state_dict sees at
 * scripts/txt2img_fgdm_inference.py:23-38 and controlnet/cldm/model.py:12-28.  Works without a GPU. */
int fgdm_param_count(const fgdm_config* cfg);
int fgdm_param_info(const fgdm_config* cfg, int index, char* name, int name_cap, int64_t* shape, int* ndim);

/* Replaces load_state_dict: copy one tensor (host or device memory, contiguous) into the engine's staging. */
int fgdm_load_tensor(fgdm_engine* e, const char* key, const void* data, int dtype, const int64_t* shape, int ndim);
/* Repack all loaded tensors into the kernel layouts (fp16, K-contiguous, GEGLU-interleaved ...) in HBM. */
int fgdm_finalize_weights(fgdm_engine* e);

/* ControlNet.input_hint_block (cldm.py:655-671,796): t-independent, so computed once per image batch and cached
 * inside the engine for ControlNet `cn`; the reference recomputes it on every apply_model call. */
int fgdm_set_hint(fgdm_engine* e, int cn, const float* hint, int B, int Hh, int Wh, void* stream);

/* LatentDiffusion.apply_model / DiffusionWrapper.forward -> UNetModel.forward (ldm/models/diffusion/ddpm.py:1035-1136,
 * 1829-1848; openaimodel.py:808-884) and, when the engine has ControlNets and FGDM_FLAG_NO_CONTROL is not set,
 * ControlLDM.apply_model (controlnet/cldm/cldm.py:836-849) using the hints cached by fgdm_set_hint:
 * eps = UNet(x, t, ctx, control = sum_k scales_k * ControlNet_k(x, hint_k, t, ctx)).
 * control_scales: n_controlnets * 13 floats (cldm.py:823) or NULL for 1.0.  pcond: optional adapter input
 * (openaimodel.py:838-841) fp32 NCHW or NULL (= x).  Timesteps: int64 `t`, or fractional fp32 `t_float` when non-NULL
 * (timestep_embedding accepts fractional t, util.py:165; DPM-Solver feeds (t_continuous - 1/N) * 1000).
 * ctx: fp32 [B,77,context_dim], or NULL to use the context registered with fgdm_set_context. */
/* AdaptUNetModel.forward(..., conds=[...]) (openaimodel.py:1263-1320): n_conds <= n_extra_adapters condition latents,
 * each fp32 NCHW [B,4,H,W] (device).  adapters[k](conds[k]) does not depend on x or t, so the summed features are
 * computed here once and added in every later fgdm_apply_model of the same B, H, W (the reference's `control` prompt is
 * fgdm_apply_model's `pcond`).  n_conds = 0 clears them (conds=None). */
int fgdm_set_adapter_conds(fgdm_engine* e, const float* const* conds, int n_conds, int B, int H, int W, void* stream);

/* The conditioning is loop-invariant (ddim.py:147-162 hands the same `cond` to every step): fgdm_set_context projects
 * ctx fp32 [B,77,context_dim] (device) through every cross-attention layer's to_k / to_v (attention.py:183-186) once;
 * fgdm_apply_model calls with ctx == NULL and the same B then reuse those projections.  A later fgdm_set_context or
 * fgdm_finalize_weights replaces / drops them. */
int fgdm_set_context(fgdm_engine* e, const float* ctx, int B, void* stream);
/* Text contexts of any length.  The reference joins the text conditioning along the token axis before the UNet sees it:
 * DiffusionWrapper.forward, cc = torch.cat(c_crossattn, 1) (ldm/models/diffusion/ddpm.py:1835-1837); ControlLDM.apply_model,
 * cond_txt = torch.cat(cond['c_crossattn'], 1) (controlnet/cldm/cldm.py:836-849); and its long-prompt route encodes every prompt
 * as three 77-token chunks, a [B,231,768] context (controlnet/cldm/hack.py:23-68).  CrossAttention takes any number of keys
 * (ldm/modules/attention.py:177-199).  fgdm_set_context_tokens states how many tokens every ctx / cond / uncond pointer passed
 * FROM NOW ON holds per sample (fgdm_set_context, fgdm_apply_model, fgdm_controlnet, fgdm_sample_ddim, fgdm_run_block): fp32
 * [B,tokens,context_dim].  Default 77.  Any tokens >= 1 is computed correctly; 64 < tokens <= 256 runs on the key-resident
 * text-attention kernels.  A changed count drops the projections registered by fgdm_set_context.  tokens < 1: FGDM_ERR_ARG.
 * All samples of a batch share the count.  No launch, no synchronisation beyond freeing the dropped projections. */
int fgdm_set_context_tokens(fgdm_engine* e, int tokens);
int fgdm_get_context_tokens(const fgdm_engine* e);
/* Cross-attention maps: what ldm/modules/attention.py:177-216 computes next to every text cross-attention and the reference's
 * inspection and editing tools start from (utils/attention_utils.py get_token_maps, utils/ptp_utils.py AttentionStore): the
 * probability every spatial query gives to every text token, averaged over heads, per transformer block, accumulated over the
 * evaluations of a sampling.  Off by default; while it is off nothing here costs a launch, an allocation or another kernel.
 *
 * fgdm_attention_capture_set registers a plan (copied; NULL: capture off, planes freed).  From then on every fgdm_apply_model --
 * and so every step of every device loop and of the per-step samplers -- runs the text cross-attention (attn2) of the selected UNet
 * blocks through the capturing instantiations of its kernel (ids 7 - 9 of fgdm_debug_last_attention_kernel; eps keeps its bits),
 * which write softmax(q k^T d^-1/2) per head in fp32; a second small kernel sums the heads IN HEAD ORDER (deterministic: no atomics),
 * picks the rows and token columns of the plan and adds the mean into (sum) or overwrites (last) the block's accumulator, fp32
 * [rows, T_block, n_tokens], T_block = the block's h * w queries in row-major order.
 *   block_mask  bit i = transformer block i of the UNet in the order of the forward pass (input blocks, middle block, output
 *               blocks: model.h, for_each_block; SD-v1 / SD-2: 0-5 down (two each at 1, 1/2, 1/4 of the latent), 6 middle, 7-15 up).
 *   tokens      n_tokens indices into the concatenated context, [0, fgdm_get_context_tokens), host; NULL with n_tokens = 0: all.
 *   rows        which rows of the batch to keep.  A CFG evaluation is ONE batch cat([uncond, cond]): FGDM_CAPTURE_ROWS_COND keeps its
 *               second half, FGDM_CAPTURE_ROWS_UNCOND its first (the batch must be even), FGDM_CAPTURE_ROWS_ALL every row.
 *   mode        FGDM_CAPTURE_SUM or FGDM_CAPTURE_LAST.
 *   batch, latent_h, latent_w   the evaluations' batch (2 B under CFG) and latent size: all three > 0 allocates the accumulators now;
 *               all three 0 leaves that to the first captured evaluation, which fixes them.  An evaluation of another shape, or
 *               after fgdm_set_context_tokens changed the count, is FGDM_ERR_STATE before any launch.
 * NOT captured: the ControlNets' cross-attentions (UNet blocks only: the tools read the UNet's), self-attention (4096^2 per head at
 * level 0), and fgdm_run_block / fgdm_controlnet, which are no evaluations of the network (the patch routes ARE, one per pass of
 * crops, and so must have the plan's shape).
 * FGDM_ERR_ARG before any launch or allocation, with the reason in fgdm_last_error: a struct_size outside
 * [FGDM_ATTENTION_CAPTURE_SIZE_V1, sizeof]; reserved0 != 0; a mask that is 0 or names a block the model does not have; n_tokens
 * outside [0, context tokens], tokens NULL with n_tokens > 0, an index outside the context; an unknown rows / mode; batch / latent
 * sizes that are negative, only partly given, or an odd batch with a half selected; and a context longer than
 * FGDM_ATTENTION_CAPTURE_MAX_KEYS tokens -- the capturing kernels' key limit -- or of 128, 192 or 256 tokens, which the dispatch
 * gives to the self-attention kernels, which have no capturing form.
 * fgdm_attention_capture_reset zeroes the accumulators and the evaluation count (asynchronous on `stream`).
 * fgdm_attention_capture_info: shape = {rows, T_block, n_tokens} of a selected block (zeros before the accumulators exist) and the
 * number of captured evaluations since the last reset; either pointer may be NULL.  fgdm_attention_capture_block_size: the block's
 * h, w (T_block = h * w).  fgdm_attention_capture_read copies the accumulated plane to dst_device (fp32, device, rows * T_block *
 * n_tokens floats) DIVIDED BY NOTHING: under FGDM_CAPTURE_SUM the caller divides by n_evals.  A block that is not selected is
 * FGDM_ERR_ARG; read before the accumulators exist is FGDM_ERR_STATE. */
#define FGDM_ATTENTION_CAPTURE_MAX_KEYS 256
#define FGDM_CAPTURE_ROWS_ALL 0
#define FGDM_CAPTURE_ROWS_COND 1
#define FGDM_CAPTURE_ROWS_UNCOND 2
#define FGDM_CAPTURE_SUM 0
#define FGDM_CAPTURE_LAST 1
#define FGDM_ATTENTION_CAPTURE_SIZE_V1 48
typedef struct fgdm_attention_capture {
    int64_t struct_size;                /* sizeof(fgdm_attention_capture) of the caller's header */
    const int32_t* tokens;              /* host, n_tokens entries, or NULL */
    uint32_t block_mask;
    int32_t n_tokens;
    int32_t rows;                       /* FGDM_CAPTURE_ROWS_* */
    int32_t mode;                       /* FGDM_CAPTURE_SUM / FGDM_CAPTURE_LAST */
    int32_t batch, latent_h, latent_w;  /* all > 0, or all 0 */
    int32_t reserved0;                  /* 0 */
} fgdm_attention_capture;
int fgdm_attention_capture_set(fgdm_engine* e, const fgdm_attention_capture* plan);
int fgdm_attention_capture_reset(fgdm_engine* e, void* stream);
int fgdm_attention_capture_info(fgdm_engine* e, int block, int64_t shape[3], int32_t* n_evals);
int fgdm_attention_capture_block_size(fgdm_engine* e, int block, int32_t* h, int32_t* w);
int fgdm_attention_capture_read(fgdm_engine* e, int block, float* dst_device, void* stream);

/* UNets fed x | c_concat: DiffusionWrapper.forward in its 'hybrid' mode, xc = torch.cat([x] + c_concat, dim=1) handed to the
 * UNet together with the text context (ldm/models/diffusion/ddpm.py:1838-1841) -- the SD-v1 inpainting checkpoints (in_channels 9:
 * latent, mask, masked-image latent) and the InstructPix2Pix family (8).  An engine created with 4 < in_channels <= 32 is such a
 * network: a plain SD UNet apart from conv_in; use_adapter and n_controlnets must be 0 (FGDM_ERR_ARG at creation otherwise, with
 * the reason in the message).  c_concat is the same tensor in every step of a sampling, so the engine keeps it: this call
 * stores c_concat fp32 NCHW [B, Cc, H, W] (device) once as fp16 NHWC [B, H W, Cc] in memory it owns (re-allocated when B, H or W
 * change; c_concat NULL drops it), and every later apply_model call packs x in front of it for conv_in (one launch, k_pack_xcat).
 * Cc must equal in_channels - 4 (FGDM_ERR_ARG otherwise, and like every refused tensor it leaves NOTHING stored: the previous
 * c_concat is dropped, so a later apply_model is FGDM_ERR_STATE rather than a run on the old image); on an engine with in_channels == 4 the call is FGDM_ERR_ARG and changes
 * nothing.  The stored rows may be the B of the later apply_model call, or B / 2 with B even: rows b and b + B / 2 then share
 * row b (the cat([x] * 2) batch of a classifier-free-guidance step whose halves carry the same image).  An apply_model call
 * without a stored c_concat, or with one whose rows or H, W do not fit, is FGDM_ERR_STATE before any launch.  With
 * FGDM_FLAG_CFG_PAIRS and B stored rows only rows [0, B / 2) of c_concat are read, like those of x.  The patch-wise
 * apply_model entry refuses such an engine (FGDM_ERR_ARG). */
int fgdm_set_concat(fgdm_engine* e, const float* c_concat, int B, int Cc, int H, int W, void* stream);
int fgdm_apply_model(fgdm_engine* e, const float* x, const int64_t* t, const float* t_float, const float* ctx,
                     const float* pcond, const float* control_scales, int B, int H, int W, int flags, float* eps_out,
                     void* stream);

/* Text conditioning: FrozenCLIPEmbedder.forward after tokenisation (ldm/modules/encoders/modules.py:153-158):
 * ids int64 [B, T] (device; T <= clip_max_len, the tokenizer's padded max_length) -> last_hidden_state fp32 [B, T, W]
 * (device).  Needs clip_layers > 0 and the cond_stage_model.transformer.text_model.* tensors loaded. */
int fgdm_clip_encode(fgdm_engine* e, const int64_t* ids, int B, int T, float* out, void* stream);
/* The long-prompt route's transformer_encode (controlnet/cldm/hack.py:40-45): clip_skip > 1 gives
 * text_model.final_layer_norm(hidden_states[-clip_skip]), i.e. the last clip_skip - 1 layers are not run (clip_skip <=
 * clip_layers + 1; hidden_states[0] are the embeddings); clip_skip <= 1 is exactly fgdm_clip_encode.  The chunked [B,231,W]
 * context of hack.py:47-68 is this call on ids [3B,77] read as [B,3*77,W] (rows (b f) -> b (f i): already contiguous). */
int fgdm_clip_encode_skip(fgdm_engine* e, const int64_t* ids, int B, int T, int clip_skip, float* out, void* stream);

/* First-stage decode: LatentDiffusion.decode_first_stage (ldm/models/diffusion/ddpm.py:832-889, plain branch) =
 * AutoencoderKL.decode(scale * z) (ldm/models/autoencoder.py:330-333; Decoder.forward,
 * ldm/modules/diffusionmodules/model.py:532-560).  z fp32 NCHW [B,4,H,W] (device), scale = 1 / scale_factor;
 * image fp32 NCHW [B, vae_out_ch, f*H, f*W], f = 2^(vae_n_levels-1).  Needs an engine created with vae_ch > 0 and the
 * first_stage_model.decoder.* / first_stage_model.post_quant_conv.* tensors loaded. */
int fgdm_vae_decode(fgdm_engine* e, const float* z, int B, int H, int W, float scale, float* image, void* stream);
/* First-stage encode: LatentDiffusion.encode_first_stage (ldm/models/diffusion/ddpm.py:952-996, plain branch) =
 * AutoencoderKL.encode (autoencoder.py:324-328): image fp32 NCHW [B,3,H,W] in [-1,1] (device) ->
 * moments fp32 NCHW [B, 2*z_channels, H/f, W/f] = DiagonalGaussianDistribution.parameters (channels [0, z_channels) the mean,
 * the rest the log-variance).  Encoder.forward (ldm/modules/diffusionmodules/model.py:436-460) then quant_conv.  H and W must be
 * multiples of f = 2^(vae_n_levels-1) and (H/f)*(W/f) a multiple of 64 (smallest image 64 x 64).  Needs an engine created with
 * vae_encoder = 1 (else FGDM_ERR_STATE) and every first_stage_model.* tensor loaded. */
int fgdm_vae_encode(fgdm_engine* e, const float* image, int B, int H, int W, float* moments, void* stream);
/* DiagonalGaussianDistribution.sample()/mode() (ldm/modules/distributions/distributions.py:24-37,61-62) times scale (the
 * scale_factor of get_first_stage_encoding, ddpm.py:660): z = scale * (mean + exp(0.5 * clamp(logvar, -30, 20)) * noise), fp32;
 * moments [B, 2*zc, HW], noise and z [B, zc, HW] (device).  noise NULL: mode(), z = scale * mean.  Stateless. */
int fgdm_posterior_sample(const float* moments, const float* noise /* NULL: mode */, float scale, float* z,
                          int B, int zc, int HW, void* stream);

/* Patch-wise evaluation of large images: the reference's `split_input_params` routes.  LatentDiffusion.get_fold_unfold
 * (ldm/models/diffusion/ddpm.py:713-763) cuts a tensor [B,C,H,W] into Ly x Lx overlapping crops of (kh, kw) cells every (sh, sw)
 * with torch.nn.Unfold -- crop l = ly * Lx + lx has its top-left corner at (ly * sh, lx * sw), Ly = (H-kh)/sh + 1, Lx = (W-kw)/sw
 * + 1 -- runs a network on every crop, multiplies the results by `weighting` (get_weighting, ddpm.py:697-711), adds them up
 * with torch.nn.Fold and divides by the folded weighting.  The weighting factors into w_pix fp32 [kh,kw] (clipped border
 * distance of a cell in its crop) and w_tie fp32 [Ly*Lx] (all ones unless `tie_braker`); weighting[.., l] = w_pix * w_tie[l],
 * rounded to fp32 once.  fgdm_amd/patches.py computes both tables; all pointers below are DEVICE pointers.
 *
 * fgdm_unfold: torch.nn.Unfold(kernel_size=(kh,kw), stride=(sh,sw)) and the view of ddpm.py:857-859 / 1056-1059, for the crops
 *   [l0, l0 + n): x fp32 [B,C,H,W] -> crops fp32 [n,B,C,kh,kw] (crop-major: one pass is a contiguous NCHW batch of n*B rows).
 * fgdm_fold_weighted: fold(o * weighting) / fold(weighting) (ddpm.py:871-877, 1123-1128) in one call: crops fp32 [L,B,C,kh,kw]
 *   for ALL L = Ly*Lx crops -> out fp32 [B,C,Ho,Wo].  Per pixel the covering crops are added in ascending l; the accumulation
 *   runs in passes of crops_per_pass crops (0: one pass) and gives the same bits for every pass size.  Unlike the reference,
 *   which returns NaN pixels there, a grid that the crops do not cover ((Ho-kh) % sh, (Wo-kw) % sw non-zero, or a stride
 *   larger than the crop) is FGDM_ERR_ARG.
 * Both are stateless, asynchronous on `stream`; every argument error is FGDM_ERR_ARG before any launch. */
int fgdm_unfold(const float* x, int B, int C, int H, int W, int kh, int kw, int sh, int sw, int l0, int n, float* crops,
                void* stream);
int fgdm_fold_weighted(const float* crops, const float* w_pix, const float* w_tie, int B, int C, int Ho, int Wo, int kh, int kw,
                       int sh, int sw, int crops_per_pass, float* out, void* stream);
/* LatentDiffusion.decode_first_stage with split_input_params['patch_distributed_vq'] (ddpm.py:841-878): z fp32 [B,4,H,W] is cut
 * into (kh, kw) latent crops every (sh, sw), every crop is decoded by AutoencoderKL.decode(scale * crop) exactly as
 * fgdm_vae_decode decodes an image of that size, and the (f kh, f kw) pixel crops are blended into image fp32
 * [B, vae_out_ch, f H, f W] with w_pix fp32 [f kh, f kw] and w_tie [Ly*Lx] (the tables at IMAGE resolution: uf = vqf = f).
 * f must equal the engine's 2^(vae_n_levels-1); kh * kw must be a multiple of 64 (the decoder's attention rule, as for
 * fgdm_vae_encode); the crops must cover the latent grid.  Crops are decoded in passes of at most max_crops_per_pass crops
 * (0: as many as fgdm_vae_decode's own images-per-pass rule allows for n*B crop images) and every pass is accumulated into
 * `image`, which is finished at the end: the activation workspace is bounded by one pass, not by H x W. */
int fgdm_vae_decode_patches(fgdm_engine* e, const float* z, int B, int H, int W, float scale, int kh, int kw, int sh, int sw,
                            int f, const float* w_pix, const float* w_tie, int max_crops_per_pass, float* image, void* stream);
/* LatentDiffusion.apply_model with split_input_params, text-conditioning branch (ddpm.py:1046-1059, 1115-1128): the UNet runs on
 * every (kh, kw) crop of x fp32 [B,4,H,W] with the SAME timesteps and context (ddpm.py:1116,1119) and the crop results are
 * blended into eps_out [B,4,H,W] with w_pix [kh,kw], w_tie [Ly*Lx].  A pass holds at most max_crops_per_pass crops (0: all) as
 * one batch of n*B rows ordered (l, b); t / t_float [B] and ctx are repeated per crop on the device.
 * ctx fp32 [B,77,context_dim] is REQUIRED (NULL: FGDM_ERR_ARG): a context registered with fgdm_set_context covers B rows, not
 * the n*B rows of a pass, so the context is taken explicitly and converted / projected per pass; the registered one is left
 * untouched.  flags: FGDM_FLAG_USE_ORIGINAL passes through; FGDM_FLAG_CFG_PAIRS is cleared (in (l, b) order the halves of the
 * batch are not the CFG halves; results are unchanged, as the flag never changes results); the ControlNet flags are ignored.
 * An engine with ControlNets is FGDM_ERR_ARG: ControlLDM.apply_model (controlnet/cldm/cldm.py:836-849) has no patch branch.
 * No pcond / conds: the reference does not forward **kwargs to the crops (ddpm.py:1119). */
int fgdm_apply_model_patches(fgdm_engine* e, const float* x, const int64_t* t, const float* t_float, const float* ctx, int B,
                             int H, int W, int kh, int kw, int sh, int sw, const float* w_pix, const float* w_tie,
                             int max_crops_per_pass, int flags, float* eps_out, void* stream);

/* Stage boundary of the two-factor chain (device pointers; byte work, bit-exact to the reference's expressions):
 *  fgdm_image_to_uint8: fp32 NCHW image -> uint8 NHWC.  mode 0 = uint8(255 * clamp((x+1)/2, 0, 1))
 *      (scripts/txt2img_fgdm_inference.py:245,249-252); mode 1 = uint8(clip(x*127.5+127.5, 0, 255))
 *      (controlnet/initialize_cn.py:101).
 *  fgdm_resize_linear_uint8: cv2.resize(img, (Wo, Ho), interpolation=cv2.INTER_LINEAR) on uint8 NHWC
 *      (scripts/txt2img_fgdm_inference.py:258; OpenCV generic fixed-point path, see oracle/boundary.py).
 *  fgdm_uint8_to_hint: control = float(img) / 255, NHWC -> fp32 NCHW (controlnet/initialize_cn.py:78-80). */
int fgdm_image_to_uint8(const float* image, int B, int C, int H, int W, int mode, uint8_t* out, void* stream);
int fgdm_resize_linear_uint8(const uint8_t* src, int B, int H, int W, int C, int Ho, int Wo, uint8_t* dst, void* stream);
int fgdm_uint8_to_hint(const uint8_t* src, int B, int H, int W, int C, float* hint, void* stream);

/* ControlNet.forward alone (cldm.py:792-813): the 13 residual tensors as fp32 NCHW, written back-to-back into
 * `out` in the order the reference returns them.  Test/inspection entry; apply_model never materialises them. */
int fgdm_controlnet(fgdm_engine* e, int cn, const float* x, const int64_t* t, const float* ctx, int B, int H, int W,
                    float* out, int64_t out_capacity_floats, void* stream);

/* One block of the loaded graph, addressed by its state-dict prefix -- the parity-test entry for the reference's block-level
 * modules: a TimestepEmbedSequential ("model.diffusion_model.input_blocks.4.", "...middle_block.", "...output_blocks.0.",
 * "control_model.input_blocks.1."; openaimodel.py:75-90) made of ResBlock (openaimodel.py:275-301), SpatialTransformer
 * (ldm/modules/attention.py:275-292), Downsample / Upsample (openaimodel.py:114-180), or the FG-DM Adapter
 * ("model.diffusion_model.adapter."; ldm/modules/encoders/adapter.py:334-346).
 * x fp32 NCHW [B,C,H,W]; x_skip: for decoder blocks the second half of th.cat([h, hs.pop()], 1) (openaimodel.py:869) fp32 NCHW
 * [B,Cs,H,W], else NULL; emb fp32 [B, 4*model_channels]: the `emb` the reference hands to the block (NULL if it has no
 * ResBlock); ctx fp32 [B,77,context_dim] (NULL if it has no SpatialTransformer).  out: fp32 NCHW (Adapter: its four
 * feature maps back to back); *out_numel = floats written. */
int fgdm_run_block(fgdm_engine* e, const char* prefix, const float* x, int C, const float* x_skip, int Cs, const float* emb,
                   const float* ctx, int B, int H, int W, float* out, int64_t out_capacity_floats, int64_t* out_numel,
                   void* stream);

/* One fused sampler update on fp32 tensors of n elements.
 * fgdm_ddim_step: p_sample_ddim's CFG combine + x_prev/pred_x0 (ldm/models/diffusion/ddim.py:243,254-268;
 * controlnet/cldm/ddim_hacked.py:192,203-231).  e_uncond NULL = no CFG; noise NULL = sigma term skipped;
 * any of x_prev / pred_x0 / e_out may be NULL. */
int fgdm_ddim_step(const float* x, const float* e_cond, const float* e_uncond, float cfg_scale, float a_t,
                   float a_prev, float sigma_t, float sqrt_one_minus_at, const float* noise, float* x_prev,
                   float* pred_x0, float* e_out, int64_t n, void* stream);
/* Adams-Bashforth eps combination of p_sample_plms (ldm/models/diffusion/plms.py:224-232); order 1..3. */
int fgdm_plms_combine(const float* e_t, const float* e1, const float* e2, const float* e3, int order,
                      float* e_prime, int64_t n, void* stream);
/* y = ca*a + cb*b (b may be NULL): the Heun-like first PLMS step (plms.py:219-223) and mask blends (ddim.py:151-154) */
int fgdm_axpby(const float* a, float ca, const float* b, float cb, float* y, int64_t n, void* stream);
/* y = a*mask + (1-mask)*b, mask already expanded to n elements: the inpainting blend of ddim.py:151-154 /
 * ldm/models/diffusion/ddpm.py:1419-1421. */
int fgdm_mask_blend(const float* a, const float* b, const float* mask, float* y, int64_t n, void* stream);
/* p_sample / p_mean_variance / q_posterior (ldm/models/diffusion/ddpm.py:284-297,1260-1323) for one timestep. */
int fgdm_ancestral_step(const float* x, const float* eps, float sqrt_recip_ac, float sqrt_recipm1_ac, float coef1,
                        float coef2, float std, const float* noise, float* out, int64_t n, void* stream);

/* Whole DDIM loop on the device (DDIMSampler.sample with eta = 0 and no host callbacks, ddim.py:58-177;
 * ddim_hacked.py:55-178).  alphas/alphas_prev/sqrt_one_minus_alphas: S floats (host) in ddim_timesteps order,
 * timesteps: S int64 (host).  cond/uncond ctx fp32 [B,77,ctx]; uncond NULL or cfg_scale == 1 disables CFG.
 * CFG runs as ONE 2B batch (cat([uncond, cond]), ddim.py:222-226); x is updated in place.
 * The entry is fgdm_sample_ddim_ex (below) with every optional field absent: same results, and the same refusals -- B, H or W <= 0
 * is FGDM_ERR_ARG with a message in fgdm_last_error(), before any launch. */
int fgdm_sample_ddim(fgdm_engine* e, float* x, const float* cond, const float* uncond, float cfg_scale, int S,
                     const int64_t* timesteps, const float* alphas, const float* alphas_prev,
                     const float* sqrt_one_minus_alphas, const float* control_scales, int B, int H, int W,
                     int flags, void* stream);

/* The whole of DDIMSampler.sample / ddim_sampling / decode without host callbacks (ldm/models/diffusion/ddim.py:58-177,
 * 395-412; controlnet/cldm/ddim_hacked.py:55-178,298-317): fgdm_sample_ddim plus stochastic steps (eta > 0, temperature), the
 * inpainting blend by mask / x0 (ddim.py:151-154), a per-step guidance scale (ucg_schedule, ddim_hacked.py:159-161) and the
 * x_inter / pred_x0 intermediates (ddim.py:171-173).  decode() from t_start is a call whose tables hold the first t_start entries.
 * fgdm_sample_ddim is this call with every optional pointer NULL.
 *
 * Per step the loop runs the network on cat([x] * 2) (or x, CFG off) and then ONE elementwise kernel (k_loop_step): CFG
 * combine, pred_x0, x_prev (+ sigma * noise), the NEXT step's blend, and the stores of x to the state and to both halves of the
 * network's input.  The arithmetic is that of fgdm_ddim_step, fgdm_axpby (q_sample) and fgdm_mask_blend, rounding for rounding:
 * the loop gives the bits of the per-step route of fgdm_amd/samplers.py fed the same noise.
 *
 * struct_size: sizeof(fgdm_ddim_params) of the CALLER's header.  Fields are only ever appended, so the library accepts every size
 * from FGDM_DDIM_PARAMS_SIZE_V1 (the struct below) up to its own sizeof and takes the fields a shorter struct lacks as zero (absent);
 * a smaller or a larger size is FGDM_ERR_ARG.  reserved0 must be 0.
 * Host tables of S entries, entry k belonging to timesteps[k] (ddim_timesteps order; the walk visits k = S-1 ... 0, ddim.py:137,148):
 *   timesteps (int64), alphas, alphas_prev, sqrt_one_minus_alphas as for fgdm_sample_ddim; sigmas (NULL: all 0, eta = 0);
 *   sqrt_alphas_cumprod_t / sqrt_one_minus_alphas_cumprod_t: q_sample's coefficients at timesteps[k] (ddpm.py:342-345), with mask only.
 * In WALK order, slot i belonging to the i-th step that runs (i = 0 is the largest timestep):
 *   cfg_scales [S] (host; NULL: cfg_scale at every step): ucg_schedule[i].  CFG is on when uncond is given and some scale is not 1;
 *     it then runs at every step, so a schedule that is 1 at SOME steps does not give the bits of a sampler that drops the
 *     unconditional half at those steps (fgdm_amd/samplers.py keeps such schedules on the per-step route);
 *   step_noise [S, B,4,H,W] (device): noise_like(x.shape) * temperature of step i (ddim.py:265-268), read at the steps whose sigma
 *     is not 0; NULL requires every sigma to be 0;
 *   mask [B,4,H,W] (device, already expanded to the latent's shape; NULL: no blending), x0 [B,4,H,W], q_noise [S, B,4,H,W]
 *     (device): in front of step i, x = q_sample(x0, t_i; q_noise[i]) * mask + (1 - mask) * x;
 *   log_steps [n_log] (host, strictly ascending walk positions in [0, S)), x_inter_out / pred_x0_out [n_log, B,4,H,W] (device, each
 *     may be NULL): slot j receives x_prev and pred_x0 of step log_steps[j] (x_prev before the next step's blend, as ddim.py:171-173
 *     appends it).  Nothing outside the n_log slots is written.
 * FGDM_ERR_ARG before any launch (x untouched): a struct_size outside that range, reserved0 != 0; a NULL x / cond / table, S, B, H or W <= 0; mask without x0,
 * q_noise or the two q_sample tables; a sigma that is not 0 without step_noise; n_log < 0, n_log > 0 without log_steps, a log step
 * outside [0, S) or not above its predecessor. */
#define FGDM_DDIM_PARAMS_SIZE_V1 192
typedef struct fgdm_ddim_params {
    int64_t struct_size;
    float* x;                           /* device [B,4,H,W]: x_T (or the latent decode() starts from) in, the sample out */
    const float* cond;                  /* device [B,tokens,context_dim] */
    const float* uncond;                /* device, or NULL */
    const int64_t* timesteps;
    const float* alphas;
    const float* alphas_prev;
    const float* sqrt_one_minus_alphas;
    const float* control_scales;        /* host, n_controlnets * 13, or NULL */
    const float* sigmas;
    const float* cfg_scales;
    const float* step_noise;
    const float* mask;
    const float* x0;
    const float* q_noise;
    const float* sqrt_alphas_cumprod_t;
    const float* sqrt_one_minus_alphas_cumprod_t;
    const int32_t* log_steps;
    float* x_inter_out;
    float* pred_x0_out;
    float cfg_scale;
    int32_t S;
    int32_t B;
    int32_t H;
    int32_t W;
    int32_t flags;                      /* FGDM_FLAG_* as for fgdm_apply_model */
    int32_t n_log;
    int32_t reserved0;                  /* 0 */
} fgdm_ddim_params;
int fgdm_sample_ddim_ex(fgdm_engine* e, const fgdm_ddim_params* p, void* stream);

/* The whole of PLMSSampler.sample / plms_sampling without host callbacks (ldm/models/diffusion/plms.py:58-236; the sampler
 * scripts/txt2img_fgdm_inference.py:183 selects with --plms).  eta is 0 (plms.py:25-26): there is no noise term.
 *
 * The walk, the table order and the slot conventions are those of fgdm_sample_ddim_ex: host tables of S entries, entry k belonging
 * to timesteps[k] (ddim_timesteps order; the walk visits k = S-1 ... 0, plms.py:138,150); q_noise and log_steps in WALK order.
 * Per network evaluation the loop launches ONE elementwise kernel (k_loop_step):
 *   step 0 (plms.py:219-223) evaluates twice.  Probe: e_t = CFG of the evaluation at timesteps[S-1] is kept as history plane 0 and
 *     x_prev = step(e_t) goes to the network's input only; the state x is untouched.  The second evaluation runs on that input at
 *     t_next = timesteps[max(S-2, 0)] (time_range[min(i + 1, len - 1)], plms.py:143: with S == 1 the same timestep again).
 *     Finish-first: e' = (e_t + e_next) / 2, rounded as the per-step route's axpby with 0.5, 0.5 rounds it.
 *   step i >= 1 (plms.py:224-232) evaluates once.  Multistep: e_t = CFG is kept as history plane i % 3 and e' is the Adams-Bashforth
 *     combination of order min(i, 3) over e_t and the planes of steps i-1, i-2, i-3, as fgdm_plms_combine computes it.  The three
 *     planes are rotated by pointer, nothing is copied: the AB order sequence is 0 (step 0), 1, 2, 3, 3, ...
 *   Every step but the probe then takes one tail: pred_x0 and x_prev from e' as fgdm_ddim_step with noise = NULL, the stores of a
 *     logged step, the NEXT step's blend (fgdm_axpby for q_sample, then fgdm_mask_blend, plms.py:145-148) and the stores of x to the
 *     state and to both halves of the network's input.
 * The arithmetic is that of fgdm_ddim_step, fgdm_plms_combine, fgdm_axpby and fgdm_mask_blend, rounding for rounding: the loop gives
 * the bits of the per-step route of fgdm_amd/samplers.py fed the same q_noise.
 *
 * CFG is on when uncond is given and cfg_scale != 1, and runs as ONE 2B batch; the loop sets FGDM_FLAG_CFG_PAIRS itself.  Hints come
 * from fgdm_set_hint; an engine with in_channels > 4 (hybrid c_concat) is refused.
 * struct_size / reserved0: as for fgdm_ddim_params, from FGDM_PLMS_PARAMS_SIZE_V1 up to the library's own sizeof.
 * mask [B,4,H,W], x0 [B,4,H,W], q_noise [S, B,4,H,W] (device) and sqrt_alphas_cumprod_t / sqrt_one_minus_alphas_cumprod_t [S] (host):
 *   as for fgdm_sample_ddim_ex.  log_steps [n_log] (host, strictly ascending walk positions in [0, S)), x_inter_out / pred_x0_out
 *   [n_log, B,4,H,W] (device, each may be NULL): slot j receives x_prev and pred_x0 of step log_steps[j] (plms.py:170-172).
 * FGDM_ERR_ARG before any launch (x untouched): a struct_size outside that range, reserved0 != 0; a NULL x / cond / table; S, B, H or
 * W <= 0; mask without x0, q_noise or the two q_sample tables; n_log < 0, n_log > 0 without log_steps, a log step outside [0, S) or
 * not above its predecessor; an engine with in_channels > 4. */
#define FGDM_PLMS_PARAMS_SIZE_V1 168
typedef struct fgdm_plms_params {
    int64_t struct_size;
    float* x;                           /* device [B,4,H,W]: x_T in, the sample out */
    const float* cond;                  /* device [B,tokens,context_dim] */
    const float* uncond;                /* device, or NULL */
    const int64_t* timesteps;
    const float* alphas;
    const float* alphas_prev;
    const float* sqrt_one_minus_alphas;
    const float* control_scales;        /* host, n_controlnets * 13, or NULL */
    const float* mask;
    const float* x0;
    const float* q_noise;
    const float* sqrt_alphas_cumprod_t;
    const float* sqrt_one_minus_alphas_cumprod_t;
    const int32_t* log_steps;
    float* x_inter_out;
    float* pred_x0_out;
    float cfg_scale;
    int32_t S;
    int32_t B;
    int32_t H;
    int32_t W;
    int32_t flags;                      /* FGDM_FLAG_* as for fgdm_apply_model */
    int32_t n_log;
    int32_t reserved0;                  /* 0 */
} fgdm_plms_params;
int fgdm_sample_plms(fgdm_engine* e, const fgdm_plms_params* p, void* stream);

/* The whole of DPMSolverSampler.sample (ldm/models/diffusion/dpm_solver/sampler.py:22-82): DPM-Solver++ (predict_x0), multistep
 * order 2, time_uniform steps, lower_order_final (dpm_solver.py:386-399 data prediction, 504-528 first-order update, 755-789
 * second-order update, 1023-1058 the multistep walk).  The sampler's mask / x0 are ignored by the reference and have no field here.
 *
 * The caller hands over one table entry per network evaluation k = 0 ... n_eval - 1 (host; n_eval is the sampler's step count S:
 * the evaluations at time_uniform t_0 ... t_{S-1}, each followed by the update to t_{k+1}):
 *   t_float[k]               the model's time input, (t_k - 1/N) * 1000 (dpm_solver.py:278-287): fractional
 *   inv_alpha[k], neg_sigma_over_alpha[k]     the data prediction m0 = inv_alpha x + neg_sigma_over_alpha eps, i.e. (x - sigma eps) / alpha
 *   update_kind[k] (int32)   FGDM_DPMPP_FIRST: x = c1 x + cm0 m0;  FGDM_DPMPP_SECOND: x = (c1 x + cm0 m0) + cm1 m1 with m1 the data
 *                            prediction of evaluation k - 1 (two roundings, the two axpby calls of the per-step route)
 *   c1[k], cm0[k], cm1[k]    the coefficients of that update as fp32 (cm1 is read for FGDM_DPMPP_SECOND only)
 * Per evaluation the loop launches ONE elementwise kernel (k_dpmpp_loop_step): CFG combine, m0 (kept in one of two planes that swap
 * by pointer), the update, and the stores of x to the state and to both halves of the network's input.  Every term is rounded as
 * fgdm_axpby rounds it: the loop gives the bits of the per-step route of fgdm_amd/samplers.py, which computes the tables with the
 * same helper (fgdm_amd.samplers.dpmpp_tables).
 * CFG, flags, hints, struct_size (from FGDM_DPMPP_PARAMS_SIZE_V1) and the reserved fields: as for fgdm_sample_plms.
 * FGDM_ERR_ARG before any launch (x untouched): a struct_size outside that range, reserved0 or reserved1 != 0; a NULL x / cond / table; n_eval, B,
 * H or W <= 0; an update_kind that is neither constant, FGDM_DPMPP_SECOND at evaluation 0; an engine with in_channels > 4. */
#define FGDM_DPMPP_FIRST 1
#define FGDM_DPMPP_SECOND 2
#define FGDM_DPMPP_PARAMS_SIZE_V1 128
typedef struct fgdm_dpmpp_params {
    int64_t struct_size;
    float* x;                           /* device [B,4,H,W]: x_T in, the sample out */
    const float* cond;                  /* device [B,tokens,context_dim] */
    const float* uncond;                /* device, or NULL */
    const float* control_scales;        /* host, n_controlnets * 13, or NULL */
    const float* t_float;
    const float* inv_alpha;
    const float* neg_sigma_over_alpha;
    const int32_t* update_kind;
    const float* c1;
    const float* cm0;
    const float* cm1;
    float cfg_scale;
    int32_t n_eval;
    int32_t B;
    int32_t H;
    int32_t W;
    int32_t flags;                      /* FGDM_FLAG_* as for fgdm_apply_model */
    int32_t reserved0;                  /* 0 */
    int32_t reserved1;                  /* 0 */
} fgdm_dpmpp_params;
int fgdm_sample_dpmpp(fgdm_engine* e, const fgdm_dpmpp_params* p, void* stream);

/* The whole of DPM_Solver.sample (ldm/models/diffusion/dpm_solver/dpm_solver.py:965-1124) for the multistep and the singlestep
 * solvers of order 1..3, noise or data prediction, as a PROGRAM: every update of the family is a linear combination of x and of model
 * values kept from earlier evaluations, and the caller expands the reference's expressions (:504-857) into those coefficients
 * (fgdm_amd.dpm_solver.dpm_solver_program).  One record per network evaluation k = 0 ... n_eval - 1 (host arrays):
 *   t_float[k]             the model's time input, (t - 1/N) * 1000 (:278-287)
 *   conv_x[k], conv_e[k]   the model value m of the record: conv_x == 0: m = eps; else m = conv_x x_eval + conv_e eps, the data
 *                          prediction (x - sigma eps) / alpha (:386-399), x_eval being the input the network just ran on
 *   slot[k] (int32)        the history plane (0..2) m is stored to, or -1: not stored
 *   nterms[k] (int32), plane[5 k + j] (int32), coef[5 k + j]      the update acc = sum_j coef_j p_j over nterms in 1..5 terms: p_j is
 *                          FGDM_DPM_PLANE_BASE (the state x), FGDM_DPM_PLANE_HIST0 + s (the history plane s, written by an earlier
 *                          record) or FGDM_DPM_PLANE_M (this record's m).  Rounding: coef_0 p_0 on its own, then every further term
 *                          fused into the sum, fma(coef_j, p_j, acc), in order
 *   dest[k] (int32)        FGDM_DPM_DEST_STATE: acc becomes the state x and the next evaluation input; FGDM_DPM_DEST_EVAL: the next
 *                          evaluation input only (the intermediate points of the singlestep solvers; x is kept)
 * Per record the loop runs the network and launches ONE elementwise kernel (k_dpm_program_step, the kernel of
 * fgdm_op_dpm_program_step): the loop gives the bits of the per-step route of fgdm_amd/dpm_solver.py over the same program.
 * CFG, flags, hints, struct_size (from FGDM_DPM_SOLVER_PARAMS_SIZE_V1) and the reserved fields: as for fgdm_sample_dpmpp.
 * FGDM_ERR_ARG before any launch (x untouched), with the offending record named in fgdm_last_error: a struct_size outside that
 * range, a reserved field != 0; a NULL x / cond / array; n_eval, B, H or W <= 0; nterms outside 1..5; an unknown plane, slot or
 * destination; a term that reads a history slot no earlier record wrote; a last record that is not FGDM_DPM_DEST_STATE; an engine
 * with in_channels > 4.  Not part of a program, so not here: method='adaptive', thresholding (both need the data on the host). */
#define FGDM_DPM_PLANE_BASE 0
#define FGDM_DPM_PLANE_HIST0 1
#define FGDM_DPM_PLANE_M 4
#define FGDM_DPM_DEST_STATE 1
#define FGDM_DPM_DEST_EVAL 2
#define FGDM_DPM_SOLVER_PARAMS_SIZE_V1 136
typedef struct fgdm_dpm_solver_params {
    int64_t struct_size;
    float* x;                           /* device [B,4,H,W]: x at t_start in, the sample out */
    const float* cond;                  /* device [B,tokens,context_dim] */
    const float* uncond;                /* device, or NULL */
    const float* control_scales;        /* host, n_controlnets * 13, or NULL */
    const float* t_float;
    const float* conv_x;
    const float* conv_e;
    const int32_t* slot;
    const int32_t* nterms;
    const int32_t* plane;               /* [n_eval * 5] */
    const float* coef;                  /* [n_eval * 5] */
    const int32_t* dest;
    float cfg_scale;
    int32_t n_eval;
    int32_t B;
    int32_t H;
    int32_t W;
    int32_t flags;                      /* FGDM_FLAG_* as for fgdm_apply_model */
    int32_t reserved0;                  /* 0 */
    int32_t reserved1;                  /* 0 */
} fgdm_dpm_solver_params;
int fgdm_sample_dpm_solver(fgdm_engine* e, const fgdm_dpm_solver_params* p, void* stream);

/* The ancestral sampler without host callbacks: LatentDiffusion.p_sample_loop / sample (ldm/models/diffusion/ddpm.py:1382-1448;
 * p_sample :1295-1323, q_posterior :290-297) over S consecutive timesteps.  There is no classifier-free guidance (p_sample has none).
 *
 * Every table and every [S, ...] tensor is in WALK order: slot i belongs to the i-th step that runs, timesteps[i] (int64, descending
 * t; p_sample_loop walks t = T-1 ... 0).  Per step the loop runs the network on x at timesteps[i] and then ONE elementwise kernel
 * (k_ancestral_loop_step):
 *   x' = fgdm_ancestral_step(x, eps, sqrt_recip_alphas_cumprod[i], sqrt_recipm1_alphas_cumprod[i], posterior_mean_coef1[i],
 *        posterior_mean_coef2[i], std[i], step_noise[i]); std[i] = temperature * exp(0.5 * posterior_log_variance_clipped[t]), and
 *        0 where t == 0 (ddpm.py:1317 nonzero_mask): such a step reads no noise, as fgdm_ancestral_step with noise = NULL.  A std
 *        of 0 at t > 0 (temperature 0) reads no noise either, while the per-step route still computes fma(0, noise, mean) there:
 *        the two can differ only in the sign of an exact zero, or where the noise is not finite;
 *   mask given: x = q mask + (1 - mask) x' with q = sqrt_alphas_cumprod_t[i] x0 + sqrt_one_minus_alphas_cumprod_t[i] q_noise[i]
 *        (fgdm_axpby, then fgdm_mask_blend).  This is the blend of the SAME step at its own timestep, applied after the update
 *        (ddpm.py:1419-1421) -- the DDIM-family loops above blend in front of the NEXT step -- so a walk may be cut into several
 *        calls at any step: the calls share nothing but x;
 *   x to the state, to the network's input and, on a logged step, to its x_inter_out slot (the x after the blend, ddpm.py:1423-1424).
 * The arithmetic is that of fgdm_ancestral_step, fgdm_axpby and fgdm_mask_blend, rounding for rounding: the loop gives the bits of
 * the per-step route of fgdm_amd/models.py fed the same noise.
 *
 * The loop clears FGDM_FLAG_CFG_PAIRS; the other flags go to the network as given.  Hints come from fgdm_set_hint; an engine with
 * in_channels > 4 (hybrid c_concat) is refused.  struct_size / reserved0 / reserved1: as for fgdm_dpmpp_params, from
 * FGDM_ANCESTRAL_PARAMS_SIZE_V1 up to the library's own sizeof.
 * step_noise [S, B,4,H,W] (device; NULL requires every std to be 0); mask [B,4,H,W], x0 [B,4,H,W], q_noise [S, B,4,H,W] (device)
 * and the two q_sample tables [S] (host): read with a mask only, which needs all of them.  log_steps [n_log] (host, strictly ascending walk positions in [0, S)),
 * x_inter_out [n_log, B,4,H,W] (device, may be NULL).
 * FGDM_ERR_ARG before any launch (x untouched): a struct_size outside that range, reserved0 or reserved1 != 0; a NULL x / cond /
 * table; S, B, H or W <= 0; mask without x0, q_noise or the two q_sample tables; a std that is not 0 without step_noise; n_log < 0,
 * n_log > 0 without log_steps, a log step outside [0, S) or not above its predecessor; an engine with in_channels > 4. */
#define FGDM_ANCESTRAL_PARAMS_SIZE_V1 176
typedef struct fgdm_ancestral_params {
    int64_t struct_size;
    float* x;                           /* device [B,4,H,W]: x_T (or the latent the walk continues from) in, the sample out */
    const float* cond;                  /* device [B,tokens,context_dim] */
    const int64_t* timesteps;
    const float* sqrt_recip_alphas_cumprod;
    const float* sqrt_recipm1_alphas_cumprod;
    const float* posterior_mean_coef1;
    const float* posterior_mean_coef2;
    const float* std;
    const float* step_noise;
    const float* control_scales;        /* host, n_controlnets * 13, or NULL */
    const float* mask;
    const float* x0;
    const float* q_noise;
    const float* sqrt_alphas_cumprod_t;
    const float* sqrt_one_minus_alphas_cumprod_t;
    const int32_t* log_steps;
    float* x_inter_out;
    int32_t S;
    int32_t B;
    int32_t H;
    int32_t W;
    int32_t flags;                      /* FGDM_FLAG_* as for fgdm_apply_model */
    int32_t n_log;
    int32_t reserved0;                  /* 0 */
    int32_t reserved1;                  /* 0 */
} fgdm_ancestral_params;
int fgdm_sample_ancestral(fgdm_engine* e, const fgdm_ancestral_params* p, void* stream);

/* DDIM inversion x_0 -> x_{t_enc} without host callbacks: DDIMSampler.encode (controlnet/cldm/ddim_hacked.py:234-279).  Host tables of S entries in walk order, slot i belonging to timesteps[i] (int64,
 * ascending t):
 *   cx[i] = sqrt(a_next / a_cur), ce[i] = sqrt(a_next) (sqrt(1 / a_next - 1) - sqrt(1 / a_cur - 1))     (ddim_hacked.py:262-266)
 * as fp32 (fgdm_amd.samplers.encode_tables computes them for both routes).  Per step the loop runs the network on cat([x] * 2) (or x,
 * CFG off) at timesteps[i] and then ONE elementwise kernel (k_invert_loop_step): e = e_uncond + cfg_scale (e_cond - e_uncond) as
 * fgdm_ddim_step's e_out, x = fgdm_axpby(x, cx[i], e, ce[i]), stored to the state, to both halves of the network's input and, on a
 * logged step, to its x_inter_out slot.  The loop gives the bits of the per-step route of fgdm_amd/samplers.py.
 * CFG (on when uncond is given and cfg_scale != 1, ONE 2B batch, FGDM_FLAG_CFG_PAIRS set by the loop), flags, hints, struct_size
 * (from FGDM_DDIM_ENCODE_PARAMS_SIZE_V1), reserved0, log_steps / x_inter_out: as for fgdm_sample_plms.
 * FGDM_ERR_ARG before any launch (x untouched): a struct_size outside that range, reserved0 != 0; a NULL x / cond / table; S, B, H or
 * W <= 0; n_log < 0, n_log > 0 without log_steps, a log step outside [0, S) or not above its predecessor; an engine with
 * in_channels > 4. */
#define FGDM_DDIM_ENCODE_PARAMS_SIZE_V1 112
typedef struct fgdm_ddim_encode_params {
    int64_t struct_size;
    float* x;                           /* device [B,4,H,W]: x_0 in, x_{t_enc} out */
    const float* cond;                  /* device [B,tokens,context_dim] */
    const float* uncond;                /* device, or NULL */
    const int64_t* timesteps;
    const float* cx;
    const float* ce;
    const float* control_scales;        /* host, n_controlnets * 13, or NULL */
    const int32_t* log_steps;
    float* x_inter_out;
    float cfg_scale;
    int32_t S;
    int32_t B;
    int32_t H;
    int32_t W;
    int32_t flags;                      /* FGDM_FLAG_* as for fgdm_apply_model */
    int32_t n_log;
    int32_t reserved0;                  /* 0 */
} fgdm_ddim_encode_params;
int fgdm_ddim_encode(fgdm_engine* e, const fgdm_ddim_encode_params* p, void* stream);

/* Device noise for the stochastic loops: a counter-based generator inside the step kernels instead of pre-drawn [S, B,4,H,W]
 * planes.  It replaces, for a caller who opts in, the host draws of ddim.py:265-268 (noise_like per step), ddpm.py:1295-1323
 * (p_sample's noise_like) and ddpm.py:342-345 (q_sample's randn_like for the inpainting blend), and util.py noise_like's
 * repeat=True; it does not reproduce torch's generator stream, and x_T stays the caller's.
 *
 * The generator is Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85) with
 *   key     = seed, low word first
 *   counter = (j >> 2, global sample index, walk position, stream id)
 * j: the element's index inside its sample (4 H W elements); global sample index = first_sample + row (0 for every row on stream 0
 * with repeat_noise); walk position = first_step + the step's position in this call (0 = the first step of the whole walk that
 * runs); stream id 0 = the sampler's step noise, 1 = q_sample's noise.  The four output words give the normals of elements
 * 4q .. 4q+3 (q = j >> 2) by Box-Muller: (r0, r1) -> (rho cos theta, rho sin theta), (r2, r3) likewise, u1 = ((r >> 8) + 1) 2^-24,
 * u2 = (r >> 8) 2^-24, rho = sqrtf(-2 logf(u1)), theta = 2 pi u2 (accurate logf / sincospif, each product rounded once).  |z| <= 5.77
 * by construction.  Stream 0's value is temperature * z, rounded once: the host's noise_like(...) * temperature; stream 1 is z.
 * So the noise of a sample at a step does not depend on how a walk is cut into calls, how a batch is sharded, or the launch.
 *
 * fgdm_loop_noise_set arms the engine with a plan (NULL: disarms; a plan replaces the one before).  While armed
 *   fgdm_sample_ddim_ex, fgdm_sample_ancestral: a NULL step_noise where a sigma / std is not 0 makes stream 0 in the step kernel;
 *   fgdm_sample_ddim_ex, fgdm_sample_plms, fgdm_sample_ancestral: a NULL q_noise with a mask makes stream 1 in the step kernel.  The
 *     DDIM-family kernels blend in front of the NEXT step and use that step's walk position, as q_noise[i + 1] is read today; the
 *     ancestral kernel blends behind the step, at its own position;
 *   a pointer that is given is read as before.  fgdm_sample_dpmpp, fgdm_sample_dpm_solver and fgdm_ddim_encode take no noise and no
 *     mask: they are not touched by the plan.
 * Unarmed, every loop behaves and fails as documented above.  FGDM_ERR_ARG from fgdm_loop_noise_set (the plan before stays): a
 * struct_size outside [FGDM_NOISE_PLAN_SIZE_V1, the library's sizeof], reserved0 / reserved1 != 0, first_sample or first_step < 0, a
 * temperature that is not finite.  FGDM_ERR_ARG from an armed loop call before any launch: first_sample + B or first_step + S above
 * INT32_MAX (the counter words are 32 bits wide). */
#define FGDM_NOISE_PLAN_SIZE_V1 40
typedef struct fgdm_noise_plan {
    int64_t struct_size;
    uint64_t seed;
    int32_t first_sample;               /* global index of row 0 of x: a rank's shard offset */
    int32_t first_step;                 /* walk position of the call's step 0: a later segment of a walk cut into calls */
    float temperature;                  /* stream 0 only; 1: plain normals */
    int32_t repeat_noise;               /* stream 0 only; not 0: every row gets sample 0's noise */
    int32_t reserved0;                  /* 0 */
    int32_t reserved1;                  /* 0 */
} fgdm_noise_plan;
int fgdm_loop_noise_set(fgdm_engine* e, const fgdm_noise_plan* plan);
/* out [B, per_sample] (device) = the numbers an armed loop makes at walk position `step` on stream `stream_id` for the rows
 * first_sample .. first_sample + B - 1 (every row sample 0 with `repeat`), times temperature: what the per-step Python route and
 * an unarmed loop are fed to give the armed loop's bits.  FGDM_ERR_ARG: a NULL out; B <= 0; per_sample <= 0 or no multiple of 4;
 * a negative stream_id, step or first_sample; first_sample + B - 1 above INT32_MAX. */
int fgdm_randn(uint64_t seed, int32_t stream_id, int32_t step, int32_t first_sample, int32_t repeat, float temperature, float* out,
               int32_t B, int32_t per_sample, void* stream);

/* Built-in kernel timer (no reference counterpart: the reference only prints wall-clock, scripts/txt2img.py:381-396).
 * Between begin and end every stride-th kernel launch is bracketed by HIP events on the launch stream
 * (work / bytes / time totals then refer to the bracketed launches only).
 * out: 4 classes x {device ms, launches, algorithmic work, algorithmic HBM bytes (igemm only)}; classes: 0 implicit GEMM (flops), 1 attention (flops),
 * 2 GroupNorm+LayerNorm (bytes), 3 im2col (bytes).  fgdm_profile_end synchronises the device. */
int fgdm_profile_begin(fgdm_engine* e, int stride /* bracket every stride-th launch; 1 = all */);
int fgdm_profile_end(fgdm_engine* e, double* out);
/* Activation workspace: peak bytes in use during the last calls, and bytes reserved from HBM. */
int fgdm_workspace_stats(fgdm_engine* e, int64_t* peak_bytes, int64_t* reserved_bytes);
/* Grouped twin launches (the UNet encoder and the ControlNets of ControlLDM.apply_model, controlnet/cldm/cldm.py:836-849, share every
 * layer shape): launches replayed from recorded walks since fgdm_create, how many of them were fused launches, and how many
 * problems those carried.  Diagnostic: the tests assert that the fused kernel really ran. */
int fgdm_launch_stats(fgdm_engine* e, int64_t* replayed_launches, int64_t* fused_launches, int64_t* fused_problems);
/* The order in which recorded walks replay, without a device (the planner behind those grouped launches, for the tests).  Walk w has
 * lens[w] units; unit u (walks concatenated) is (key[u], grid_x[u], shape[u]), key 0 = it has no grouped form.  The walks are cut
 * into runs of `chunk` (<= 0: one run) as fgdm_apply_model cuts them by FGDM_GROUP_MAX, and every run is scheduled for grouped
 * launches of up to `group_max` (>= 1) members.  out receives the steps, each  n, (walk, unit) x n : n == 1 a unit on its own,
 * n >= 2 one grouped launch; at most out_cap values are written.  Returns the number of values of the whole schedule (< 0: bad
 * arguments); limits (may be NULL) receives [0] how many of a walk's pending units are searched for a group's member and [1] the
 * largest group the engine launches (FGDM_MAX_GROUP). */
int fgdm_replay_plan(int n_walks, const int32_t* lens, const uint64_t* key, const uint32_t* grid_x, const uint64_t* shape,
                     int group_max, int chunk, int32_t* out, int out_cap, int* limits);

/* Per-kernel entry points used by the parity tests (tests/test_gpu_ops.py); weights given in the reference's
 * native layouts (fp32, [Cout,Cin,kh,kw] / [N,K]) and packed on the fly.  Activations fp16 NHWC.
 * fgdm_op_conv2d `stride`: 1, 2 (padding 1 on every side), or FGDM_STRIDE2_PAD_BR: stride 2 with the zero padding on the bottom
 * and right only -- the first-stage encoder's Downsample (ldm/modules/diffusionmodules/model.py:72-76: F.pad(x, (0,1,0,1)) then
 * conv3x3 stride 2 padding 0), ksize 3 only; out is [B, (H-2)/2+1, (W-2)/2+1, Cout]. */
#define FGDM_STRIDE2_PAD_BR (-2)
int fgdm_op_conv2d(const void* x0, int C0, const void* x1, int C1, const float* w, const float* bias,
                   const float* rowvec, const void* resid, int B, int H, int W, int Cout, int ksize, int stride,
                   int upsample, int act, float scale, void* out, void* stream);
int fgdm_op_linear(const void* x, const float* w, const float* bias, const void* resid, int M, int K, int N,
                   int act, int out_kind, int rows_per_sample, int ld_out, void* out, void* stream);
/* Producer / consumer pair of a transformer-block LayerNorm (ldm/modules/attention.py:234-240: attn(norm(x)), ff(norm(x))) as
 * the engine evaluates it: h = x W1^T + b1 (+ resid) is written as fp16 [M, C] together with per-row partial sums, and
 * y = act(LayerNorm(h; gamma, beta, eps 1e-5) W2^T + b2) runs on the RAW h with the LayerNorm folded into W2 and applied to
 * the fp32 accumulator (no normalised copy of h exists).  x fp16 [M, K1], resid fp16 [M, C] or NULL, weights fp32 in the
 * reference's [out, in] layout, act2 0 or 3 (GEGLU: y is [M, N2 / 2]).  *slots_used: partial-sum slots per row. */
int fgdm_op_linear_ln_linear(const void* x, const float* w1, const float* b1, const void* resid, const float* gamma,
                             const float* beta, const float* w2, const float* b2, int M, int K1, int C, int N2, int act2,
                             void* h_out, void* y_out, int* slots_used, void* stream);
/* Tuning aids: force the implicit-GEMM tile configuration process-wide (0 = automatic; 1-3 = 2-stage kernel
 * 128x128 / 128x64 / 64x64; 4-6 = pipelined kernel 256x320 / 256x256 / 128x320), and time one conv / linear shape on
 * random data (average device milliseconds over `iters` launches). */
int fgdm_debug_force_igemm_cfg(int cfg);
int fgdm_bench_igemm(int B, int H, int W, int C0, int C1, int Cout, int ksize, int stride, int upsample, int act,
                     int use_resid, int cfg, int iters, float* avg_ms);
/* ... one attention shape (softmax(QK^T d^-1/2) V over B x heads, T queries, Tk keys) ... */
/* tools/bench_ff.py: GEGLU projection + output projection of a feed-forward block (ldm/modules/attention.py:37-64) in row
 * chunks sharing one intermediate buffer; average device milliseconds for all M rows. */
int fgdm_bench_ff(int M, int C, int chunk_rows, int iters, float* avg_ms);
int fgdm_bench_attention(int B, int heads, int T, int Tk, int d, int iters, float* avg_ms);
/* ... the same shape through the capturing instantiation (cross-attention maps: the per-head planes written), with_reduce: followed
 * by the head reduction into maps [B, T, Tk]; FGDM_ERR_ARG where fgdm_op_cross_attention_maps is. */
int fgdm_bench_attention_maps(int B, int heads, int T, int Tk, int d, int with_reduce, int iters, float* avg_ms);
/* ... and one GroupNorm32(+SiLU) (kind 0, optional virtual concat C1) or LayerNorm (kind 1) shape. */
int fgdm_bench_norm(int kind, int B, int HW, int C0, int C1, int silu, int iters, float* avg_ms);
int fgdm_op_groupnorm(const void* x0, int C0, const void* x1, int C1, int B, int HW, const float* gamma,
                      const float* beta, float eps, int silu, void* out, void* stream);
int fgdm_op_layernorm(const void* x, int rows, int C, const float* gamma, const float* beta, float eps,
                      void* out, void* stream);
/* O[b, t, h d + :] = softmax(Q K^T d^-1/2) V, all fp16: Q [B, T, ldq], K [B, Tk, ldk] (head h at columns [h d, (h+1) d) of a row;
 * ldq, ldk multiples of 8, ldo of 4; columns of a row beyond heads * d are never read, and never written in O), V transposed:
 * vt [B, heads * d, ldvt], keys contiguous, ldvt a multiple of 8 and >= roundup(Tk, 64).  Contract for the columns of a V^T row:
 * [0, Tk) the values; [Tk, roundup(Tk, 64)) must be ZERO (the kernels load whole 32- / 64-key tiles and multiply the pad
 * columns by probabilities that are exactly 0, so anything finite would do, a NaN or Inf would not); columns >=
 * roundup(Tk, 64) are read by no kernel and may hold anything.  d is 40, 64, 80 or 160. */
int fgdm_op_attention(const void* q, int ldq, const void* k, int ldk, const void* vt, int ldvt, void* o, int ldo,
                      int B, int heads, int T, int Tk, int d, void* stream);
/* Diagnostic entries (tests/test_gpu_attention_calls.py); the product path does not call them.
 * fgdm_op_attention_ex: fgdm_op_attention with the engine's q_prescaled flag passed through.  q_prescaled = 1: Q already carries
 * log2(e) d^-1/2 (the engine folds it into the to_q weights), so O = softmax(ln 2 * Q K^T) V and the kernels scale by exactly 1.
 * fgdm_debug_last_attention_kernel: which kernel the dispatch chose on the last successful attention call of this process:
 * 0 none yet, 1 general (attn_kernel), 2 text-token (attn_cross_kernel<D, 3>), 3 long-text (attn_cross_kernel<D, 4 ... 8>), 4 ping-pong
 * (attn_pp_kernel), 5 two-strand 16-wide (attn_two_strand_kernel<D, Pv16<D>>), 6 two-strand 32-wide (attn_two_strand_kernel<D, Pv32<D>>).
 * fgdm_op_small_attention: the text encoder's attention, softmax(q k^T d^-1/2 (j <= i when causal)) v with q | k | v as column
 * blocks of one fp16 [B T, ld] matrix (q at column 0, k at koff, v at voff; head h at columns [64 h, 64 h + 64) of its block),
 * out fp16 [B T, ldo]; d = 64 and 1 <= T <= 128, anything else is FGDM_ERR_ARG before any launch. */
int fgdm_op_attention_ex(const void* q, int ldq, const void* k, int ldk, const void* vt, int ldvt, void* o, int ldo,
                         int B, int heads, int T, int Tk, int d, int q_prescaled, void* stream);
int fgdm_debug_last_attention_kernel(void);
/* Diagnostic entry (tests/test_gpu_attention_maps.py): fgdm_op_attention_ex through the CAPTURING instantiations of the two kernels
 * that take text contexts, which besides O write the probabilities; maps fp32 [B, T, Tk] (device) is
 *   maps[b, t, k] = mean over heads of softmax_k(q k^T d^-1/2)[b, h, t, k],
 * from the fp32 exponentials before they are rounded to fp16 for the P V product, normalised by their own fp32 sum; heads are summed
 * in head order by a second kernel, so two calls give the same bits.  O has the bits fgdm_op_attention_ex gives.  The dispatch is
 * that of fgdm_op_attention_ex; fgdm_debug_last_attention_kernel then reports 7 general capturing (attn_kernel), 8 text-token
 * capturing (attn_cross_kernel<D, 3>), 9 long-text capturing (attn_cross_kernel<D, 4 ... 8>).  FGDM_ERR_ARG before any launch: a NULL
 * pointer; B, heads, T or Tk <= 0; Tk > FGDM_ATTENTION_CAPTURE_MAX_KEYS; another d; a shape the dispatch gives to a self-attention kernel
 * (ids 4 - 6: these have no capturing form).  Allocates B heads T Tk floats of scratch and synchronises the stream. */
int fgdm_op_cross_attention_maps(const void* q, int ldq, const void* k, int ldk, const void* vt, int ldvt, void* o, int ldo, float* maps,
                                 int B, int heads, int T, int Tk, int d, int q_prescaled, void* stream);
int fgdm_op_small_attention(const void* qkv, int ld, int koff, int voff, void* out, int ldo, int B, int heads, int T, int d,
                            int causal, void* stream);

/* Diagnostic entries (tests/test_gpu_narrow_ops.py); the product path does not call them.  Every argument error is FGDM_ERR_ARG
 * before any launch.
 *
 * fgdm_op_conv2d with (C0 + C1) % 64 != 0 -- the first convolution of every network: UNet / ControlNet conv_in, the adapter input,
 * ControlNet.input_hint_block up to its 256-wide layer (controlnet/cldm/cldm.py:655-671), the first-stage conv_in's (ldm/modules/
 * diffusionmodules/model.py:390,484).  Accepted for ksize == 3, C1 == 0 (x1 NULL), upsample == 0 and stride 1 or 2, the combinations
 * the engine's own im2col route takes; anything else stays FGDM_ERR_ARG.  C0 is the logical Cin; x0 is fp16 NHWC with cin_pad
 * channels, cin_pad = roundup(Cin, 8) when Cin % 8 == 0, else roundup(Cin, 4).  Contract for the pad channels [Cin, cin_pad) of
 * x0: they must be FINITE (the engine's layout kernel leaves them +0); their columns of the packed weight are exactly zero, so a
 * finite value there changes no bit of the result.  w is [Cout, Cin, 3, 3] fp32; all epilogue arguments work as for Cin % 64 == 0.
 *
 * fgdm_op_vae_attention: the core of the first-stage AttnBlock (ldm/modules/diffusionmodules/model.py:176-203, lines 188-199: ONE
 * head over all C channels), per image b: out_b = softmax(C^-1/2 q_b k_b^T) v_b, as the engine evaluates it (fp32 scores by a GEMM
 * with the K rows as weight, row softmax to fp16, a GEMM over T with V^T as weight).  All fp16: q [B T, C]; k [B T + 128, C];
 * vt [B, C, T] (V transposed, tokens contiguous); out [B T, C].  T and C multiples of 64.  Contract for the 128 rows after the last
 * key row of k: they must be readable and FINITE (the GEMM loads whole weight tiles of up to 128 rows; the rows beyond an image's
 * T keys -- the next image's keys, or this pad -- feed only score columns >= T, which are never written); what follows them is
 * read by no kernel.  vt: when C is a multiple of 128 nothing beyond [B, C, T] is read and anything may follow; otherwise up to 64
 * further rows of T halves after the last image's V^T must be readable (they feed only output columns >= C, never written). */
int fgdm_op_vae_attention(const void* q, const void* k, const void* vt, void* out, int B, int T, int C, void* stream);
/* One entry per kernel of the layout / elementwise group, on caller-owned device buffers; asynchronous on `stream`.
 *  fgdm_op_softmax_rows: P = fp16(softmax(S)) over the `cols` fp32 logits of each of `rows` rows (AttnBlock, model.py:190-192).
 *  fgdm_op_nchw_to_nhwc: x fp32 [B, C, HW] -> y fp16 [B, HW, Cpad], channels >= C exactly +0 (Cpad >= C).
 *  fgdm_op_nhwc_to_nchw: x fp16 [B, HW, C] -> y fp32 [B, C, HW].
 *  fgdm_op_pack_xcat (tests/test_gpu_hybrid.py): the first-layer input of an engine with in_channels > 4, as apply_model packs it:
 *      x fp32 [B, 4, H W] and cc16 fp16 [Bc, H W, Cc] (the layout the engine stores c_concat in) -> out fp16 [B, H W, cin_pad]:
 *      channels [0, 4) x, [4, 4 + Cc) row b % Bc of cc16, [4 + Cc, cin_pad) exactly +0.  Bc = B, or B / 2 with B even; cin_pad a
 *      multiple of 4 and >= 4 + Cc (the engine passes roundup(4 + Cc, 8) when 4 + Cc is a multiple of 8, else roundup(4 + Cc, 4)).
 *  fgdm_op_avgpool2: AvgPool2d(2) on fp16 NHWC [B, H, W, C] -> [B, H/2, W/2, C] (the adapter's Downsample with use_conv = False,
 *      ldm/modules/encoders/adapter.py:270-273); H, W even, C a multiple of 8.
 *  fgdm_op_transpose_pad: v fp16 [B, Tk, C] -> vt fp16 [B, C, Tkpad], columns [Tk, Tkpad) exactly zero (Tkpad >= Tk).
 *  fgdm_op_timestep_embed: timestep_embedding (ldm/modules/diffusionmodules/util.py:160-180): y fp16 [rows_pad, dim], row b < B =
 *      [cos(t_b f_k) | sin(t_b f_k)], f_k = exp(-ln(1e4) k / (dim / 2)); t int64 [B], or fp32 t_float [B] when non-NULL ("these may be
 *      fractional", util.py:165); rows [B, rows_pad) exactly zero.  dim even.
 *  fgdm_op_add_f16: y = a + b on n fp16 elements, summed in fp32 and rounded once; n a multiple of 8; y may alias a. */
int fgdm_op_softmax_rows(const float* S, void* P, int rows, int cols, void* stream);
int fgdm_op_nchw_to_nhwc(const float* x, void* y, int B, int C, int HW, int Cpad, void* stream);
int fgdm_op_nhwc_to_nchw(const void* x, float* y, int B, int C, int HW, void* stream);
int fgdm_op_pack_xcat(const float* x, const void* cc16, int B, int Bc, int Cc, int H, int W, int cin_pad, void* out, void* stream);
int fgdm_op_avgpool2(const void* x, void* y, int B, int H, int W, int C, void* stream);
int fgdm_op_transpose_pad(const void* v, void* vt, int B, int Tk, int C, int Tkpad, void* stream);
int fgdm_op_timestep_embed(const int64_t* t, const float* t_float, void* y, int B, int dim, int rows_pad, void* stream);
int fgdm_op_add_f16(const void* a, const void* b, void* y, int64_t n, void* stream);

/* Diagnostic entries (tests/test_gpu_fp32_ops.py); the product path does not call them.  One entry per fp32-side kernel of the text
 * encoder and of the first stage, on caller-owned device buffers; asynchronous on `stream`.  Every argument error -- a NULL
 * pointer, a count <= 0, what each entry names below -- is FGDM_ERR_ARG before any launch.
 *  fgdm_op_embed_tokens: out fp32 [rows, W], row r = tok[clamp(ids[r], 0, vocab - 1)] + pos[r % T]: CLIPTextEmbeddings on int64 ids
 *      [rows = B T], fp32 tables tok [vocab, W] and pos [>= T, W], one fp32 add per element.  W a multiple of 8.
 *  fgdm_op_layernorm32: LayerNorm over the C columns of each of `rows` fp32 rows (two-pass fp32 statistics, biased variance),
 *      gamma / beta fp32 [C], stored as fp16 to out16 or as fp32 to out32: exactly one of the two non-NULL.  C a multiple of 4.
 *  fgdm_op_add_f16_to_f32: y = a + float(b16) on n elements (a, y fp32; b16 fp16): the residual add of a CLIP layer.
 *  fgdm_op_f32_to_f16: y = fp16(x) on n elements, round to nearest even (the context upload).
 *  fgdm_op_silu_f32_to_f16: y = fp16(x sigmoid(x)) on n elements, evaluated in fp32 (`emb` handed in from outside).
 *  fgdm_op_vae_prequant: post_quant_conv (1x1, 4 -> 4; ldm/models/autoencoder.py:331) on scale z with the layout change:
 *      z fp32 [B, 4, HW] -> y fp16 [B, HW, 4], y[b, p, co] = fp16(wb[16 + co] + sum_ci wb[4 co + ci] (scale z[b, ci, p])); wb fp32 [20].
 *  fgdm_op_vae_moments: quant_conv (1x1, 8 -> 8; autoencoder.py:326) with the layout change: h fp32 [B, HW, 8] (16-byte aligned)
 *      -> moments fp32 [B, 8, HW], moments[b, co, p] = wb[64 + co] + sum_ci wb[8 co + ci] h[b, p, ci]; wb fp32 [72]. */
int fgdm_op_embed_tokens(const int64_t* ids, const float* tok, const float* pos, float* out, int rows, int T, int W, int vocab,
                         void* stream);
int fgdm_op_layernorm32(const float* x, int rows, int C, const float* gamma, const float* beta, float eps, void* out16, float* out32,
                        void* stream);
int fgdm_op_add_f16_to_f32(const float* a, const void* b16, float* y, int64_t n, void* stream);
int fgdm_op_f32_to_f16(const float* x, void* y, int64_t n, void* stream);
int fgdm_op_silu_f32_to_f16(const float* x, void* y, int64_t n, void* stream);
int fgdm_op_vae_prequant(const float* z, const float* wb, float scale, void* y, int B, int HW, void* stream);
int fgdm_op_vae_moments(const float* h, const float* wb, float* moments, int B, int HW, void* stream);

/* Diagnostic entry (tests/test_gpu_ddim_loop.py); only fgdm_sample_ddim_ex's loop launches this kernel in the product path.
 *
 * fgdm_op_ddim_loop_step: one launch of k_loop_step in its plain mode, the per-step kernel of fgdm_sample_ddim_ex, on n fp32 elements:
 *   e = e_uncond + cfg_scale (e_cond - e_uncond) (e_uncond NULL: e_cond); pred_x0 and x_prev exactly as fgdm_ddim_step (ddim.py:243,
 *   254-268; noise NULL: no sigma term) -> log_pred_x0, log_x (each may be NULL);
 *   mask given: x = q mask + (1 - mask) x_prev with q = sqrt_ac_next x0 + sqrt_one_minus_ac_next q_noise (ddim.py:151-154: the blend
 *   in front of the NEXT step, fgdm_axpby then fgdm_mask_blend rounding for rounding); mask NULL: x = x_prev;
 *   x -> x_out, xin_a, xin_b (each may be NULL; x_out may be x itself, no other buffers may overlap).
 *   e_cond NULL: no update, x_prev = x (the launch in front of the first step).
 * FGDM_ERR_ARG before any launch: x NULL, n <= 0, e_uncond without e_cond, mask without x0 or q_noise. */
int fgdm_op_ddim_loop_step(const float* x, const float* e_cond, const float* e_uncond, float cfg_scale, float a_t, float a_prev,
                           float sigma_t, float sqrt_one_minus_at, const float* noise, const float* mask, const float* x0,
                           const float* q_noise, float sqrt_ac_next, float sqrt_one_minus_ac_next, float* x_out, float* xin_a,
                           float* xin_b, float* log_x, float* log_pred_x0, int64_t n, void* stream);

/* Diagnostic entries (tests/test_gpu_multistep_loop.py); only the loops of fgdm_sample_plms / fgdm_sample_dpmpp launch these kernels
 * in the product path.  n fp32 elements; every output may be NULL (nothing is written) and nothing outside n elements is written.
 *
 * fgdm_op_plms_loop_step: one launch of k_loop_step in a PLMS mode.  e = e_uncond + cfg_scale (e_cond - e_uncond) (e_uncond NULL: e_cond)
 *   -> e_out in every mode (the loop passes NULL in mode 1), then
 *   mode 0 (probe, plms.py:219-221): x_prev of e, exactly as fgdm_ddim_step with noise NULL -> xin_a, xin_b; x_out, the
 *     logs and the blend are not touched;
 *   mode 1 (finish-first, plms.py:222-223): e' = 0.5 e1 + 0.5 e rounded as fgdm_axpby rounds it (e1: the probe's e_t);
 *   mode 2 (multistep, plms.py:224-232): e' = the combination of fgdm_plms_combine over e, e1, e2, e3 for order 1..3
 *     (e_out may be e3 itself);
 *   modes 1 and 2: pred_x0, x_prev from e' as fgdm_ddim_step -> log_pred_x0, log_x; mask given: x = q mask + (1 - mask) x_prev with
 *     q = sqrt_ac_next x0 + sqrt_one_minus_ac_next q_noise (fgdm_axpby then fgdm_mask_blend), else x = x_prev; x -> x_out, xin_a, xin_b
 *     (x_out may be x itself).  e_cond NULL: no update, x_prev = x (the launch in front of the first step).
 *   FGDM_ERR_ARG before any launch: x NULL, n <= 0, e_uncond without e_cond, mask without x0 or q_noise, an unknown mode, mode 1
 *   without e1, mode 2 with an order outside 1..3 or without the planes of that order.
 * fgdm_op_dpmpp_loop_step: one launch of k_dpmpp_loop_step.  m0 = inv_alpha x + neg_sigma_over_alpha e -> m0_out; update_kind
 *   FGDM_DPMPP_FIRST: x = c1 x + cm0 m0; FGDM_DPMPP_SECOND: x = (c1 x + cm0 m0) + cm1 m1; each sum rounded as fgdm_axpby rounds it
 *   (dpm_solver.py:386-399, 504-528, 755-789); x -> x_out, xin_a, xin_b (x_out may be x itself).
 *   FGDM_ERR_ARG before any launch: x or e_cond NULL, n <= 0, another update_kind, FGDM_DPMPP_SECOND without m1. */
int fgdm_op_plms_loop_step(const float* x, const float* e_cond, const float* e_uncond, float cfg_scale, int mode, int order,
                           const float* e1, const float* e2, const float* e3, float* e_out, float a_t, float a_prev,
                           float sqrt_one_minus_at, const float* mask, const float* x0, const float* q_noise, float sqrt_ac_next,
                           float sqrt_one_minus_ac_next, float* x_out, float* xin_a, float* xin_b, float* log_x, float* log_pred_x0,
                           int64_t n, void* stream);
int fgdm_op_dpmpp_loop_step(const float* x, const float* e_cond, const float* e_uncond, float cfg_scale, float inv_alpha,
                            float neg_sigma_over_alpha, const float* m1, int update_kind, float c1, float cm0, float cm1,
                            float* m0_out, float* x_out, float* xin_a, float* xin_b, int64_t n, void* stream);

/* fgdm_op_dpm_program_step: one launch of k_dpm_program_step on caller-owned buffers of n fp32 elements -- what the per-step route of
 * fgdm_amd/dpm_solver.py launches behind every network evaluation, and what fgdm_sample_dpm_solver launches per record.
 *   e = e_uncond + cfg_scale (e_cond - e_uncond) (e_uncond NULL: e_cond);  m = e (conv_x == 0) or conv_x x_eval + conv_e e, rounded as
 *   fgdm_axpby rounds it;  m -> the history plane `slot` (hist0..2; -1: not stored);  acc = coefs[0] p_0, then fma(coefs[j], p_j, acc)
 *   for j = 1 .. nterms - 1, p_j by planes[j]: FGDM_DPM_PLANE_BASE `base`, FGDM_DPM_PLANE_HIST0 + s `hist<s>`, FGDM_DPM_PLANE_M the m
 *   of this launch;  acc -> x_out, xin_a, xin_b (each may be NULL; nothing outside n elements is written).  planes / coefs: host.
 *   Element i of every plane is read before anything is written at i, by the same thread: x_out may be base, the slot's plane may be
 *   one a term reads, xin_a may be x_eval.  Planes that overlap in any other way are not allowed.
 *   FGDM_ERR_ARG before any launch: n <= 0; nterms outside 1..5; planes or coefs NULL; an unknown plane or slot; a NULL plane that a
 *   term or the slot names; e_cond NULL; x_eval NULL with conv_x != 0. */
int fgdm_op_dpm_program_step(const float* x_eval, const float* e_cond, const float* e_uncond, float cfg_scale, float conv_x, float conv_e,
                             float* base, float* hist0, float* hist1, float* hist2, int slot, int nterms, const int32_t* planes,
                             const float* coefs, float* x_out, float* xin_a, float* xin_b, int64_t n, void* stream);

/* Diagnostic entries (tests/test_gpu_ancestral_loop.py); only the loops of fgdm_sample_ancestral / fgdm_ddim_encode launch these
 * kernels in the product path.  n fp32 elements; every output may be NULL and nothing outside n elements is written.
 *
 * fgdm_op_ancestral_loop_step: one launch of k_ancestral_loop_step.  x' exactly as fgdm_ancestral_step (noise NULL or std == 0: no
 *   noise term); mask given: x = q mask + (1 - mask) x' with q = sqrt_ac_t x0 + sqrt_one_minus_ac_t q_noise (fgdm_axpby then
 *   fgdm_mask_blend: the blend of the SAME step), else x = x'; x -> x_out, xin, log_x (x_out may be x itself).
 *   FGDM_ERR_ARG before any launch: x or eps NULL, n <= 0, mask without x0 or q_noise.
 * fgdm_op_invert_loop_step: one launch of k_invert_loop_step.  e = e_uncond + cfg_scale (e_cond - e_uncond) (e_uncond NULL: e_cond),
 *   x = cx x + ce e rounded as fgdm_axpby rounds it; x -> x_out, xin_a, xin_b, log_x (x_out may be x itself).
 *   FGDM_ERR_ARG before any launch: x or e_cond NULL, n <= 0. */
int fgdm_op_ancestral_loop_step(const float* x, const float* eps, float sqrt_recip_ac, float sqrt_recipm1_ac, float coef1, float coef2,
                                float std, const float* noise, const float* mask, const float* x0, const float* q_noise,
                                float sqrt_ac_t, float sqrt_one_minus_ac_t, float* x_out, float* xin, float* log_x, int64_t n,
                                void* stream);
int fgdm_op_invert_loop_step(const float* x, const float* e_cond, const float* e_uncond, float cfg_scale, float cx, float ce,
                             float* x_out, float* xin_a, float* xin_b, float* log_x, int64_t n, void* stream);

/* Diagnostic entry (tests/test_gpu_device_noise.py): the raw words of the loops' generator (fgdm_loop_noise_set).
 * out [n_blocks, 4] uint32 (device): row k = Philox4x32-10, key = seed (low word first), of the 128-bit counter (c0 lowest word)
 * + k, carries into the higher words included.  FGDM_ERR_ARG: out NULL, n_blocks <= 0. */
int fgdm_op_rand_bits(uint64_t seed, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t* out, int64_t n_blocks, void* stream);

/* Diagnostic entry (tests/test_gpu_qkv_projection.py); the product path does not call it.
 *
 * fgdm_op_ln_qkv: to_q | to_k | to_v of a self-attention (ldm/modules/attention.py:180-186: three Linear(C, C, bias=False)) behind
 * norm1 (attention.py:238), as the ONE GEMM the engine launches for them (Engine::attn_fwd): the stacked weight [3C, C] over the
 * tokens h with two destinations -- packed columns [0, 2C) row-major to qk, columns [2C, 3C) TRANSPOSED to vt (IgemmArgs::out2,
 * out_kind2 = OUT_F16_T, ld_out2 = Tp, split_n = 2C, rows_per_sample = T, M = B T, N = 3C, K = C, no activation, scale 1) -- through
 * igemm_launch, so the automatic tile choice and fgdm_debug_force_igemm_cfg both apply.
 *   h fp16 [B T, C];  wq / wk / wv fp32 [C, C] in the reference's [out, in] layout (host or device), no bias;
 *   qk fp16 [B T, 2C] (q at columns [0, C), k at [C, 2C));  vt fp16 [B, C, Tp], tokens contiguous.
 * fold = 1: h holds the RAW tokens and LayerNorm(gamma, beta fp32 [C], eps 1e-5) is folded into the GEMM as in
 *   fgdm_op_linear_ln_linear's consumer: weight fp16(gamma_k w_nk), the bias carries beta W, the per-row partial sums of h come
 *   from the separate row-statistics pass (C / 160 slots) and (mean, rstd) are applied to the fp32 accumulator of BOTH destinations.
 * fold = 0: gamma and beta must be NULL, h is taken as already normalised (the FGDM_LN_FOLD=0 engine) and the weights are packed
 *   plain.
 * The entry does NOT clear vt: the columns [T, Tp) of every V^T row are the caller's (the engine zeroes them once; the GEMM writes
 * around them) and are left untouched.  FGDM_ERR_ARG before any launch for a NULL h / wq / wk / wv / qk / vt; B, T or C <= 0;
 * C % 320 != 0 (split_n = 2C must be a multiple of 640, the launcher's rule); Tp < T; Tp % 8 != 0; gamma / beta not matching
 * `fold`; B T 3C beyond 2^31 - 1.  A forced tile the launcher refuses for the shape (e.g. 256 x 256 tiles when 3C % 256 != 0) is
 * FGDM_ERR_ARG as well, with qk and vt untouched. */
int fgdm_op_ln_qkv(const void* h, const float* gamma, const float* beta, const float* wq, const float* wk, const float* wv,
                   int B, int T, int C, int Tp, int fold, void* qk, void* vt, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------------
 * Weight updates of a FINALIZED engine (LoRA adapters and the like): selected parameters are supplied again as fp32 in device
 * memory and the packed layers that own them are re-packed in place, through the packer fgdm_finalize_weights runs -- so every
 * fold (stacked q | k | v with norm1 and the query scale, the GEGLU pair with norm3, conv layouts, the stacked emb_layers and text
 * projections) applies as it did at the first packing.  No packed buffer moves; what the engine had computed from weights and kept
 * (the registered context's K / V^T, the summed adapter features, the ControlNets' hint-block outputs) is dropped by a commit and
 * by a restore: call fgdm_set_context / fgdm_set_adapter_conds / fgdm_set_hint again (a call that needs one is refused by name
 * until then, never served stale).
 *
 * A packed layer is built from several parameters -- a weight and its bias, the LayerNorm folded into a Linear, q, k and v of one
 * attention, every emb_layers Linear of a network.  A commit needs ALL parameters of every layer it touches;
 * fgdm_weights_update_plan lists them without a device.
 *
 *   fgdm_weights_begin_update    opens an update, forgetting tensors of an unfinished one.
 *   fgdm_weights_update_tensor   one parameter, fp32 in device (or host) memory, complete when the call is made (synchronise the
 *                                stream that produced it); copied to host staging, the caller's buffer is free on return.
 *   fgdm_weights_commit_update   waits for `stream`, re-packs, ends the update.  Synchronous.
 *   fgdm_weights_snapshot        keeps a device copy of the packed bytes of the layers that own `keys`; layers already held keep
 *                                their FIRST copy, so the snapshot stays the state before any update.
 *   fgdm_weights_restore         waits for `stream`, puts the snapshot back byte for byte and releases it.
 *   fgdm_weights_snapshot_bytes  device memory the snapshot holds now.
 *
 * Refusals leave the packed weights as they were: FGDM_ERR_STATE for an engine that is not finalized, an update_tensor or commit
 * without begin_update, a restore without a snapshot; FGDM_ERR_ARG for an unknown key, a rank or shape that differs from the
 * registered one, and a commit with a partly supplied packed layer (the message names the missing key; the update is over and its
 * tensors are forgotten).  fgdm_finalize_weights after new fgdm_load_tensor calls drops the snapshot.
 *
 * fgdm_weights_update_plan: the packed layers owning any of `keys`, as text in `out`: one layer per line, its keys separated by one
 * blank.  Returns the bytes needed including the final NUL (nothing is written when out_cap is smaller), FGDM_ERR_ARG for an
 * unknown key (named by fgdm_last_error of NULL). */
int fgdm_weights_begin_update(fgdm_engine* e);
int fgdm_weights_update_tensor(fgdm_engine* e, const char* key, const float* device_fp32, const int64_t* shape, int ndim);
int fgdm_weights_commit_update(fgdm_engine* e, void* stream);
int fgdm_weights_snapshot(fgdm_engine* e, const char* const* keys, int n);
int fgdm_weights_restore(fgdm_engine* e, void* stream);
int64_t fgdm_weights_snapshot_bytes(const fgdm_engine* e);
int fgdm_weights_update_plan(const fgdm_config* cfg, const char* const* keys, int n, char* out, int out_cap);

/* fgdm_op_lora_merge: out[o, i] = W[o, i] + s sum_{k < r} up[o, k] down[k, i] over fp32 device buffers W, out [O, I], up [O, r],
 * down [r, I]; a conv weight is taken as [Cout, Cin kh kw].  Per element: acc = 0, then acc = fmaf(up[o, k], down[k, i], acc) for
 * k = 0 .. r - 1 in that order, then fmaf(s, acc, W[o, i]) -- the same bits whatever the launch.  out may be W.
 * FGDM_ERR_ARG before any launch: a NULL pointer, O or I <= 0, r outside 1..128. */
int fgdm_op_lora_merge(const float* W, const float* up, const float* down, float s, int O, int I, int r, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
