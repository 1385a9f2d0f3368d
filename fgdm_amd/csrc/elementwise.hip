// Small HBM-bound kernels of the hot path: layout/dtype conversion at the API boundary, im2col for the
// few convolutions whose Cin is not a multiple of 64, 2x2 average pooling (FG-DM adapter), sinusoidal
// timestep embedding, and the fused sampler updates (CFG combine + DDIM / PLMS / ancestral step).
#include "common.h"

#define EW_BLOCK 256
static inline int ew_grid(size_t n) {
    size_t g = (n + EW_BLOCK - 1) / EW_BLOCK;
    return (int)(g > 4096 ? 4096 : (g < 1 ? 1 : g));
}
#define EW_LOOP(i, n) for (size_t i = (size_t)blockIdx.x * EW_BLOCK + threadIdx.x; i < (n); i += (size_t)gridDim.x * EW_BLOCK)
#define LAUNCH_OK() (hipGetLastError() == hipSuccess ? FGDM_OK : FGDM_ERR_HIP)

// x [B, C, HW] fp32  ->  y [B, HW, Cpad] fp16 (channels >= C zero)
__global__ void k_nchw_to_nhwc(const float* __restrict__ x, half_t* __restrict__ y, int B, int C, int HW, int Cpad) {
    const size_t n = (size_t)B * HW * Cpad;
    EW_LOOP(i, n) {
        const int c = (int)(i % Cpad);
        const size_t bp = i / Cpad;
        const size_t b = bp / HW, p = bp - b * HW;
        y[i] = c < C ? (half_t)x[(b * C + c) * HW + p] : (half_t)0;
    }
}
int nchw_f32_to_nhwc_f16(const float* x, half_t* y, int B, int C, int HW, int Cpad, hipStream_t s) {
    FGDM_LAUNCH(k_nchw_to_nhwc, dim3(ew_grid((size_t)B * HW * Cpad)), dim3(EW_BLOCK), 0, s, x, y, B, C, HW, Cpad);
    return LAUNCH_OK();
}

// First-layer input of a UNet fed cat([x] + c_concat, 1) (DiffusionWrapper 'hybrid', ldm/models/diffusion/ddpm.py:1838-1841):
// x [B, 4, HW] fp32 | cc [Bc, HW, Cc] fp16 (the engine's cached c_concat)  ->  y [B, HW, Cpad] fp16: channels [0, 4) from x (rounded
// as k_nchw_to_nhwc rounds), [4, 4 + Cc) from row b % Bc of cc (Bc = B, or B / 2: both halves of a CFG batch share a row),
// [4 + Cc, Cpad) zero.  One thread per pixel row: the x loads of a wave are contiguous per channel; G halves per store
// (G = 8 when Cpad % 8 == 0, else 4).
template <int G>
__global__ void k_pack_xcat(const float* __restrict__ x, const half_t* __restrict__ cc, half_t* __restrict__ y, int B, int Bc,
                            int Cc, int HW, int Cpad) {
    typedef half_t vec_t __attribute__((ext_vector_type(G)));
    const size_t n = (size_t)B * HW;
    EW_LOOP(i, n) {
        const size_t b = i / HW, p = i - b * HW;
        const float* xr = x + b * 4 * HW + p;
        const half_t* cr = cc + ((b % Bc) * HW + p) * Cc;
        half_t* yr = y + i * Cpad;
        for (int c0 = 0; c0 < Cpad; c0 += G) {
            vec_t v;
#pragma unroll
            for (int e = 0; e < G; ++e) {
                const int c = c0 + e;
                v[e] = c < 4 ? (half_t)xr[(size_t)c * HW] : (c < 4 + Cc ? cr[c - 4] : (half_t)0);
            }
            *(vec_t*)(yr + c0) = v;
        }
    }
}
int pack_xcat(const float* x, const half_t* cc, half_t* y, int B, int Bc, int Cc, int HW, int Cpad, hipStream_t s) {
    if (B <= 0 || Bc <= 0 || Cc <= 0 || HW <= 0 || Cpad < 4 + Cc || (Cpad & 3) || !(Bc == B || (B % 2 == 0 && Bc == B / 2)))
        return FGDM_ERR_ARG;
    if ((Cpad & 7) == 0) {
        FGDM_LAUNCH(k_pack_xcat<8>, dim3(ew_grid((size_t)B * HW)), dim3(EW_BLOCK), 0, s, x, cc, y, B, Bc, Cc, HW, Cpad);
    } else {
        FGDM_LAUNCH(k_pack_xcat<4>, dim3(ew_grid((size_t)B * HW)), dim3(EW_BLOCK), 0, s, x, cc, y, B, Bc, Cc, HW, Cpad);
    }
    return LAUNCH_OK();
}

__global__ void k_f32_to_f16(const float* __restrict__ x, half_t* __restrict__ y, size_t n) {
    EW_LOOP(i, n) y[i] = (half_t)x[i];
}
int f32_to_f16(const float* x, half_t* y, size_t n, hipStream_t s) {
    FGDM_LAUNCH(k_f32_to_f16, dim3(ew_grid(n)), dim3(EW_BLOCK), 0, s, x, y, n);
    return LAUNCH_OK();
}
__global__ void k_nhwc_f16_to_nchw_f32(const half_t* __restrict__ x, float* __restrict__ y, int B, int C, int HW) {
    const size_t n = (size_t)B * C * HW;
    EW_LOOP(i, n) {
        const int p = (int)(i % HW);
        const size_t bc = i / HW;
        const int c = (int)(bc % C);
        const size_t b = bc / C;
        y[i] = (float)x[(b * HW + p) * C + c];
    }
}
int nhwc_f16_to_nchw_f32(const half_t* x, float* y, int B, int C, int HW, hipStream_t s) {
    FGDM_LAUNCH(k_nhwc_f16_to_nchw_f32, dim3(ew_grid((size_t)B * C * HW)), dim3(EW_BLOCK), 0, s, x, y, B, C, HW);
    return LAUNCH_OK();
}
// y = fp16(SiLU(x)): the `emb_layers` input of a ResBlock (openaimodel.py:238-244) when `emb` is handed in from outside
__global__ void k_silu_f32_to_f16(const float* __restrict__ x, half_t* __restrict__ y, size_t n) {
    EW_LOOP(i, n) { const float v = x[i]; y[i] = (half_t)silu_f(v); }
}
int silu_f32_to_f16(const float* x, half_t* y, size_t n, hipStream_t s) {
    FGDM_LAUNCH(k_silu_f32_to_f16, dim3(ew_grid(n)), dim3(EW_BLOCK), 0, s, x, y, n);
    return LAUNCH_OK();
}

// A[m][k], k = tap * C + c (k < 9C), zero for k in [9C, Kpad); 3x3 window, pad 1, given stride.
// G = channels per thread-granule (8 when C % 8 == 0, else 4 for C == 4)
template <int G>
__global__ void k_im2col(const half_t* __restrict__ x, half_t* __restrict__ A, int B, int H, int W, int C,
                         int stride, int Ho, int Wo, int Kpad) {
    typedef half_t vec_t __attribute__((ext_vector_type(G)));
    const int KG = Kpad / G;
    const size_t n = (size_t)B * Ho * Wo * KG;
    EW_LOOP(i, n) {
        const int kg = (int)(i % KG);
        const size_t m = i / KG;
        const int k = kg * G;
        vec_t v = (vec_t)(half_t)0;
        if (k < 9 * C) {
            const int tap = k / C, c = k - tap * C;
            const int ky = tap / 3, kx = tap - ky * 3;
            const int hw = Ho * Wo;
            const int b = (int)(m / hw), rem = (int)(m - (size_t)b * hw);
            const int oy = rem / Wo, ox = rem - oy * Wo;
            const int iy = oy * stride + ky - 1, ix = ox * stride + kx - 1;
            if ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W)
                v = *(const vec_t*)(x + (((size_t)b * H + iy) * W + ix) * C + c);
        }
        *(vec_t*)(A + m * Kpad + k) = v;
    }
}
int im2col3x3(const half_t* x, half_t* A, int B, int H, int W, int C, int stride, int Kpad, hipStream_t s) {
    const int Ho = (H + 2 - 3) / stride + 1, Wo = (W + 2 - 3) / stride + 1;
    if (Kpad < 9 * C || (Kpad & 63)) return FGDM_ERR_ARG;
    if ((C & 7) == 0) {
        FGDM_LAUNCH(k_im2col<8>, dim3(ew_grid((size_t)B * Ho * Wo * (Kpad / 8))), dim3(EW_BLOCK), 0, s, x, A, B,
                           H, W, C, stride, Ho, Wo, Kpad);
    } else if ((C & 3) == 0) {
        FGDM_LAUNCH(k_im2col<4>, dim3(ew_grid((size_t)B * Ho * Wo * (Kpad / 4))), dim3(EW_BLOCK), 0, s, x, A, B,
                           H, W, C, stride, Ho, Wo, Kpad);
    } else {
        return FGDM_ERR_ARG;
    }
    return LAUNCH_OK();
}

// AvgPool2d(2) on NHWC fp16 (ldm/modules/encoders/adapter.py:270-273, use_conv=False)
__global__ void k_avgpool2(const half_t* __restrict__ x, half_t* __restrict__ y, int B, int H, int W, int C) {
    const int Ho = H / 2, Wo = W / 2, P = C / 8;
    const size_t n = (size_t)B * Ho * Wo * P;
    EW_LOOP(i, n) {
        const int o = (int)(i % P);
        const size_t m = i / P;
        const int hw = Ho * Wo;
        const int b = (int)(m / hw), rem = (int)(m - (size_t)b * hw);
        const int oy = rem / Wo, ox = rem - oy * Wo;
        const half_t* p = x + (((size_t)b * H + 2 * oy) * W + 2 * ox) * C + o * 8;
        const h8 a = *(const h8*)p, bq = *(const h8*)(p + C), c = *(const h8*)(p + (size_t)W * C),
                 d = *(const h8*)(p + (size_t)W * C + C);
        h8 r;
#pragma unroll
        for (int e = 0; e < 8; ++e) r[e] = (half_t)(0.25f * ((float)a[e] + (float)bq[e] + (float)c[e] + (float)d[e]));
        *(h8*)(y + m * C + o * 8) = r;
    }
}
int avgpool2(const half_t* x, half_t* y, int B, int H, int W, int C, hipStream_t s) {
    if ((C & 7) || (H & 1) || (W & 1)) return FGDM_ERR_ARG;
    FGDM_LAUNCH(k_avgpool2, dim3(ew_grid((size_t)B * (H / 2) * (W / 2) * (C / 8))), dim3(EW_BLOCK), 0, s, x, y, B, H, W, C);
    return LAUNCH_OK();
}

__global__ void k_add_f16(const half_t* __restrict__ a, const half_t* __restrict__ b, half_t* __restrict__ y, size_t n8) {
    EW_LOOP(i, n8) {
        const h8 u = ((const h8*)a)[i], v = ((const h8*)b)[i];
        h8 r;
#pragma unroll
        for (int e = 0; e < 8; ++e) r[e] = (half_t)((float)u[e] + (float)v[e]);
        ((h8*)y)[i] = r;
    }
}
int add_f16(const half_t* a, const half_t* b, half_t* y, size_t n, hipStream_t s) {
    if (n & 7) return FGDM_ERR_ARG;
    FGDM_LAUNCH(k_add_f16, dim3(ew_grid(n / 8)), dim3(EW_BLOCK), 0, s, a, b, y, n / 8);
    return LAUNCH_OK();
}

// y[b] = [cos(t f_i) | sin(t f_i)], f_i = exp(-ln(1e4) i / half)   (util.py:160-180); rows >= B are zero
// y = a + float(b): a fp16 branch output added to the fp32 residual stream (CLIP's hidden states under autocast promote)
__global__ void k_add_f16_to_f32(const float* __restrict__ a, const half_t* __restrict__ b, float* __restrict__ y, size_t n) {
    EW_LOOP(i, n) y[i] = a[i] + (float)b[i];
}
int add_f16_to_f32(const float* a, const half_t* b, float* y, size_t n, hipStream_t s) {
    FGDM_LAUNCH(k_add_f16_to_f32, dim3(ew_grid(n)), dim3(EW_BLOCK), 0, s, a, b, y, n);
    return LAUNCH_OK();
}

__global__ void k_timestep_embed(const int64_t* __restrict__ t, const float* __restrict__ tf, half_t* __restrict__ y,
                                 int B, int dim, int rows_pad) {
    const int half = dim / 2;
    const size_t n = (size_t)rows_pad * dim;
    EW_LOOP(i, n) {
        const int b = (int)(i / dim), j = (int)(i % dim);
        float v = 0.f;
        if (b < B) {
            const int k = j < half ? j : j - half;
            const float f = expf(-9.210340371976184f * (float)k / (float)half);
            const float arg = (tf ? tf[b] : (float)t[b]) * f;      // "These may be fractional" (util.py:165): DPM-Solver
            v = j < half ? cosf(arg) : sinf(arg);
        }
        y[i] = (half_t)v;
    }
}
int timestep_embed(const int64_t* t, const float* tf, half_t* y, int B, int dim, int rows_pad, hipStream_t s) {
    FGDM_LAUNCH(k_timestep_embed, dim3(ew_grid((size_t)rows_pad * dim)), dim3(EW_BLOCK), 0, s, t, tf, y, B, dim, rows_pad);
    return LAUNCH_OK();
}

// v [B, Tk, C] -> vt [B, C, Tkpad] (zero for t >= Tk); used once per sample() call for the context V of cross-attention
__global__ void k_transpose_pad(const half_t* __restrict__ v, half_t* __restrict__ vt, int B, int Tk, int C, int Tkpad) {
    const size_t n = (size_t)B * C * Tkpad;
    EW_LOOP(i, n) {
        const int t = (int)(i % Tkpad);
        const size_t bc = i / Tkpad;
        const size_t b = bc / C, c = bc - b * C;
        vt[i] = t < Tk ? v[(b * Tk + t) * C + c] : (half_t)0;
    }
}
int transpose_pad_keys(const half_t* v, half_t* vt, int B, int Tk, int C, int Tkpad, hipStream_t s) {
    FGDM_LAUNCH(k_transpose_pad, dim3(ew_grid((size_t)B * C * Tkpad)), dim3(EW_BLOCK), 0, s, v, vt, B, Tk, C, Tkpad);
    return LAUNCH_OK();
}

// ---------------------------------------------------------------- sampler updates (fp32, one fused pass)
// e = e_u + s (e_c - e_u)                                        ldm/models/diffusion/ddim.py:243
// pred_x0 = (x - sqrt(1-a_t) e) / sqrt(a_t)                      ddim.py:259
// x_prev  = sqrt(a_prev) pred_x0 + sqrt(1 - a_prev - sigma^2) e + sigma * noise     ddim.py:263-268
//
// The loop step kernels further down must give the bits of the per-step kernels they fuse (k_ddim_step, k_plms, k_axpby,
// k_mask_blend), and this file is compiled with -ffp-contract=fast, under which an expression's source does not say which products
// are fused into a sum (a `*` behind __fmul_rn included).  So each formula is written ONCE, here, with every rounding explicit --
// __builtin_fmaf where the product is fused, mul_rn where it is rounded on its own -- and both sets of kernels call it: they agree
// by construction, under any compiler.  tests/test_gpu_sampler_update_bits.py pins the bits themselves.
__device__ __forceinline__ float mul_rn(float a, float b) {
    float p = a * b;
    asm volatile("" : "+v"(p));     // no instruction: the product is a value in a register, so it cannot become the multiplicand of an FMA
    return p;
}
__device__ __forceinline__ float cfg_combine_rn(float ec, float eu, float s) { return __builtin_fmaf(s, ec - eu, eu); }
__device__ __forceinline__ float ddim_dir_rn(float a_prev, float sigma) { return sqrtf(__builtin_fmaf(-sigma, sigma, 1.0f - a_prev)); }
__device__ __forceinline__ float pred_x0_rn(float x, float e, float s1m, float sa) { return __builtin_fmaf(-s1m, e, x) / sa; }
__device__ __forceinline__ float x_prev_rn(float p0, float e, float sp, float dir) { return mul_rn(dir, e) + mul_rn(sp, p0); }
__device__ __forceinline__ float add_noise_rn(float xp, float sigma, float noise) { return __builtin_fmaf(sigma, noise, xp); }
__device__ __forceinline__ float axpby_rn(float ca, float a, float cb, float b) { return __builtin_fmaf(ca, a, mul_rn(cb, b)); }
__device__ __forceinline__ float mask_blend_rn(float a, float b, float m) { return mul_rn(a, m) + mul_rn(1.0f - m, b); }
// Adams-Bashforth combinations of plms.py:224-232; order = number of old eps available (1..3); e2 / e3 are read from order 2 / 3 on
__device__ __forceinline__ float adams_bashforth_rn(int order, float e, const float* e1, const float* e2, const float* e3, size_t i) {
    if (order == 1) return mul_rn(__builtin_fmaf(3.f, e, -e1[i]), 0.5f);
    if (order == 2) return (__builtin_fmaf(-16.f, e1[i], mul_rn(23.f, e)) + mul_rn(5.f, e2[i])) / 12.f;
    return (((mul_rn(55.f, e) - mul_rn(59.f, e1[i])) + mul_rn(37.f, e2[i])) - mul_rn(9.f, e3[i])) / 24.f;
}

__global__ void k_ddim_step(const float* __restrict__ x, const float* __restrict__ ec, const float* __restrict__ eu,
                            float cfg, float a_t, float a_prev, float sigma, float s1m, const float* __restrict__ noise,
                            float* __restrict__ x_prev, float* __restrict__ pred_x0, float* __restrict__ e_out, size_t n) {
    const float sa = sqrtf(a_t), sp = sqrtf(a_prev), dir = ddim_dir_rn(a_prev, sigma);
    EW_LOOP(i, n) {
        float e = ec[i];
        if (eu) e = cfg_combine_rn(e, eu[i], cfg);
        const float p0 = pred_x0_rn(x[i], e, s1m, sa);
        float xp = x_prev_rn(p0, e, sp, dir);
        if (noise) xp = add_noise_rn(xp, sigma, noise[i]);
        if (x_prev) x_prev[i] = xp;
        if (pred_x0) pred_x0[i] = p0;
        if (e_out) e_out[i] = e;
    }
}
int ddim_step(const float* x, const float* e_cond, const float* e_uncond, float cfg_scale, float a_t, float a_prev,
              float sigma_t, float sqrt_one_minus_at, const float* noise, float* x_prev, float* pred_x0, float* e_out,
              size_t n, hipStream_t s) {
    FGDM_LAUNCH(k_ddim_step, dim3(ew_grid(n)), dim3(EW_BLOCK), 0, s, x, e_cond, e_uncond, cfg_scale, a_t, a_prev,
                       sigma_t, sqrt_one_minus_at, noise, x_prev, pred_x0, e_out, n);
    return LAUNCH_OK();
}

// The two ends every loop step kernel shares (StepIO, common.h): the network's e at element i (ec, or the CFG combine of k_ddim_step
// where eu is given), and the stores of the new x to the state and to both halves of the network's cat([x] * 2) input.  The log store
// stays with each kernel: they log different values.
__device__ __forceinline__ float step_eps(const StepIO& io, size_t i) {
    float e = io.ec[i];
    if (io.eu) e = cfg_combine_rn(e, io.eu[i], io.cfg);
    return e;
}
__device__ __forceinline__ void step_store(const StepIO& io, size_t i, float xn) {
    if (io.x_out) io.x_out[i] = xn;
    if (io.xin_a) io.xin_a[i] = xn;
    if (io.xin_b) io.xin_b[i] = xn;
}
// ... and the host check of the I/O in front of every launch; need_ec: the kernel has no mode without an update
static bool step_io_ok(const StepIO& io, bool need_ec = true, bool need_x = true) {
    return (io.x || !need_x) && io.n != 0 && (io.ec || (!need_ec && !io.eu));
}
// The next step's inpainting blend (k_axpby, then k_mask_blend; ddim.py:151-154), then the shared store: the tail of k_loop_step.
__device__ __forceinline__ void loop_blend_store(const LoopStep& a, size_t i, float xp) {
    float xn = xp;
    if (a.mask) xn = mask_blend_rn(axpby_rn(a.sa_next, a.x0[i], a.s1m_next, a.qnoise ? a.qnoise[i] : noise_q(a.gen, i)), xp, a.mask[i]);
    step_store(a.io, i, xn);
}
// ... and the host check of a step's generator (noise.h): off, or whole samples of a multiple of four elements
static bool noise_gen_ok(const NoiseGen& g, size_t n) {
    return (!g.step_on && !g.q_on) || (g.per_sample != 0 && g.per_sample % 4 == 0 && n % g.per_sample == 0);
}

// One launch per network evaluation of the device DDIM and PLMS loops (fgdm_sample_ddim_ex, fgdm_sample_plms), one pass over the n
// elements.  e_t = e_u + s (e_c - e_u) -> e_out, then by mode
//   plain         e' = e_t                                                                          ddim.py:243
//   probe         e' = e_t;  x_prev = step(e') -> the two input halves only, nothing else           plms.py:219-221
//   finish-first  e' = (e1 + e_t) / 2 with e1 the probe's e_t, as k_axpby(e1, 0.5, e_t, 0.5)        plms.py:222-223
//   multistep     e' = k_plms(e_t, e1, e2, e3, order)                                               plms.py:224-232
// then pred_x0 / x_prev from e' as k_ddim_step (sigma * noise included; the PLMS loop leaves them 0 / NULL), the logged stores
// (x_prev BEFORE the next step's blend, as the per-step loop appends it) and loop_blend_store.  ec NULL: no update, x_prev = x (the
// blend and the input copies in front of the first step).  e_out may be e3 (read before it is written, as StepIO says of x).
__global__ void k_loop_step(const LoopStep a) {
    const float sa = sqrtf(a.a_t), sp = sqrtf(a.a_prev), dir = ddim_dir_rn(a.a_prev, a.sigma);
    EW_LOOP(i, a.io.n) {
        float xp = a.io.x[i];
        if (a.io.ec) {
            const float e = step_eps(a.io, i);
            float ep = e;
            if (a.mode == LOOP_FINISH_FIRST) ep = axpby_rn(0.5f, a.e1[i], 0.5f, e);
            else if (a.mode == LOOP_MULTISTEP) ep = adams_bashforth_rn(a.order, e, a.e1, a.e2, a.e3, i);
            if (a.e_out) a.e_out[i] = e;
            const float p0 = pred_x0_rn(xp, ep, a.s1m, sa);
            xp = x_prev_rn(p0, ep, sp, dir);
            if (a.noise) xp = add_noise_rn(xp, a.sigma, a.noise[i]);
            else if (a.gen.step_on) xp = add_noise_rn(xp, a.sigma, noise_step(a.gen, i));
            if (a.mode == LOOP_PROBE) {
                if (a.io.xin_a) a.io.xin_a[i] = xp;
                if (a.io.xin_b) a.io.xin_b[i] = xp;
                continue;
            }
            if (a.io.log_x) a.io.log_x[i] = xp;
            if (a.log_p0) a.log_p0[i] = p0;
        }
        loop_blend_store(a, i, xp);
    }
}
int loop_step(const LoopStep& a, hipStream_t s) {
    if (!step_io_ok(a.io, false) || (a.mask && (!a.x0 || (!a.qnoise && !a.gen.q_on))) || !noise_gen_ok(a.gen, a.io.n)) return FGDM_ERR_ARG;
    if (a.io.ec) {
        if (a.mode != LOOP_PLAIN && a.mode != LOOP_PROBE && a.mode != LOOP_FINISH_FIRST && a.mode != LOOP_MULTISTEP) return FGDM_ERR_ARG;
        if (a.mode == LOOP_FINISH_FIRST && !a.e1) return FGDM_ERR_ARG;
        if (a.mode == LOOP_MULTISTEP && (a.order < 1 || a.order > 3 || !a.e1 || (a.order >= 2 && !a.e2) || (a.order >= 3 && !a.e3)))
            return FGDM_ERR_ARG;
    }
    FGDM_LAUNCH(k_loop_step, dim3(ew_grid(a.io.n)), dim3(EW_BLOCK), 0, s, a);
    return LAUNCH_OK();
}

// One launch per network evaluation of the device DPM-Solver++ loop (fgdm_sample_dpmpp; dpm_solver.py:386-399, 504-528, 755-789):
//   m0 = k_axpby(x, inv_alpha, CFG, neg_sigma_over_alpha) -> m0_out
//   first order   x = k_axpby(x, c1, m0, cm0)
//   second order  x = k_axpby(k_axpby(x, c1, m0, cm0), 1, m1, cm1)
// and x to the state and to both halves of the network's input.
__global__ void k_dpmpp_loop_step(const DpmppLoopStep a) {
    EW_LOOP(i, a.io.n) {
        const float xi = a.io.x[i];
        const float e = step_eps(a.io, i);
        const float m0 = axpby_rn(a.inv_alpha, xi, a.neg_sigma_over_alpha, e);
        if (a.m0_out) a.m0_out[i] = m0;
        float xn = axpby_rn(a.c1, xi, a.cm0, m0);
        if (a.kind == DPMPP_SECOND) xn = axpby_rn(1.0f, xn, a.cm1, a.m1[i]);
        step_store(a.io, i, xn);
    }
}
int dpmpp_loop_step(const DpmppLoopStep& a, hipStream_t s) {
    if (!step_io_ok(a.io) || (a.kind != DPMPP_FIRST && a.kind != DPMPP_SECOND) || (a.kind == DPMPP_SECOND && !a.m1)) return FGDM_ERR_ARG;
    FGDM_LAUNCH(k_dpmpp_loop_step, dim3(ew_grid(a.io.n)), dim3(EW_BLOCK), 0, s, a);
    return LAUNCH_OK();
}

// The linear combination of a DPM-Solver program record: the first product rounded on its own, every further term fused into the
// sum, in the record's order.
__device__ __forceinline__ float lincomb_rn(const float* c, const float* p, int nterms) {
    float acc = mul_rn(c[0], p[0]);
#pragma unroll
    for (int j = 1; j < DPM_MAX_TERMS; ++j)
        if (j < nterms) acc = __builtin_fmaf(c[j], p[j], acc);
    return acc;
}
// One launch per network evaluation of the device DPM-Solver program loop (fgdm_sample_dpm_solver) and of the per-step route
// (fgdm_op_dpm_program_step): the model value m of the record (eps, or the data prediction of dpm_solver.py:386-399), kept in its
// history slot, and the record's update as a linear combination of up to five planes (dpm_solver.py:504-857 expanded on the host).
// No __restrict__: an output may be one of the input planes, so every load of element i comes before the first store to it.
__global__ void k_dpm_program_step(const DpmProgramStep a) {
    EW_LOOP(i, a.io.n) {
        const float e = step_eps(a.io, i);
        const float m = a.conv_x == 0.f ? e : axpby_rn(a.conv_x, a.io.x[i], a.conv_e, e);
        float p[DPM_MAX_TERMS];
#pragma unroll
        for (int j = 0; j < DPM_MAX_TERMS; ++j) p[j] = (j < a.nterms && a.term[j]) ? a.term[j][i] : m;
        const float acc = lincomb_rn(a.coef, p, a.nterms);
        if (a.m_out) a.m_out[i] = m;
        step_store(a.io, i, acc);
    }
}
int dpm_program_terms(DpmProgramStep& a, float* const planes[4], int slot, int nterms, const int32_t* src, const float* coef) {
    if (nterms < 1 || nterms > DPM_MAX_TERMS || !src || !coef || slot < -1 || slot > 2) return FGDM_ERR_ARG;
    for (int j = 0; j < DPM_MAX_TERMS; ++j) { a.term[j] = nullptr; a.coef[j] = 0.f; }
    for (int j = 0; j < nterms; ++j) {
        if (src[j] < DPM_PLANE_BASE || src[j] > DPM_PLANE_M) return FGDM_ERR_ARG;
        if (src[j] != DPM_PLANE_M && !planes[src[j]]) return FGDM_ERR_ARG;
        a.term[j] = src[j] == DPM_PLANE_M ? nullptr : planes[src[j]];
        a.coef[j] = coef[j];
    }
    a.nterms = nterms;
    a.m_out = nullptr;
    if (slot >= 0) {
        if (!planes[DPM_PLANE_HIST0 + slot]) return FGDM_ERR_ARG;
        a.m_out = planes[DPM_PLANE_HIST0 + slot];
    }
    return FGDM_OK;
}
int dpm_program_step(const DpmProgramStep& a, hipStream_t s) {
    if (!step_io_ok(a.io, true, a.conv_x != 0.f) || a.nterms < 1 || a.nterms > DPM_MAX_TERMS) return FGDM_ERR_ARG;
    FGDM_LAUNCH(k_dpm_program_step, dim3(ew_grid(a.io.n)), dim3(EW_BLOCK), 0, s, a);
    return LAUNCH_OK();
}

__global__ void k_plms(const float* __restrict__ e, const float* __restrict__ e1, const float* __restrict__ e2,
                       const float* __restrict__ e3, int order, float* __restrict__ out, size_t n) {
    EW_LOOP(i, n) out[i] = adams_bashforth_rn(order, e[i], e1, e2, e3, i);
}
int plms_combine(const float* e_t, const float* e1, const float* e2, const float* e3, int order, float* e_prime,
                 size_t n, hipStream_t s) {
    if (order < 1 || order > 3) return FGDM_ERR_ARG;
    FGDM_LAUNCH(k_plms, dim3(ew_grid(n)), dim3(EW_BLOCK), 0, s, e_t, e1, e2, e3, order, e_prime, n);
    return LAUNCH_OK();
}

__global__ void k_axpby(const float* __restrict__ a, float ca, const float* __restrict__ b, float cb,
                        float* __restrict__ y, size_t n) {
    EW_LOOP(i, n) y[i] = b ? axpby_rn(ca, a[i], cb, b[i]) : ca * a[i] + 0.f;
}
int axpby(const float* a, float ca, const float* b, float cb, float* y, size_t n, hipStream_t s) {
    FGDM_LAUNCH(k_axpby, dim3(ew_grid(n)), dim3(EW_BLOCK), 0, s, a, ca, b, cb, y, n);
    return LAUNCH_OK();
}

// inpainting blend img_orig * mask + (1 - mask) * img (ddim.py:151-154, ddpm.py:1419-1421); mask pre-expanded
__global__ void k_mask_blend(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ m,
                             float* __restrict__ y, size_t n) {
    EW_LOOP(i, n) y[i] = mask_blend_rn(a[i], b[i], m[i]);
}
int mask_blend(const float* a, const float* b, const float* m, float* y, size_t n, hipStream_t s) {
    FGDM_LAUNCH(k_mask_blend, dim3(ew_grid(n)), dim3(EW_BLOCK), 0, s, a, b, m, y, n);
    return LAUNCH_OK();
}

// ancestral step (ddpm.py:284-297, 1318-1323): x0 = c_r x - c_rm1 eps; mean = c1 x0 + c2 x; out = mean + std * noise.
// Written once for k_ancestral and k_ancestral_loop_step, like the helpers above: c_rm1 eps is fused into c_r x, the two products
// of the mean are rounded on their own, std * noise is fused into the mean (noise NULL: the t == 0 step, no noise term).
__device__ __forceinline__ float ancestral_rn(float x, float eps, float cr, float crm1, float c1, float c2, float std,
                                              const float* noise, size_t i) {
    const float x0 = __builtin_fmaf(-crm1, eps, mul_rn(cr, x));
    float r = mul_rn(c1, x0) + mul_rn(c2, x);
    if (noise) r = add_noise_rn(r, std, noise[i]);
    return r;
}
__global__ void k_ancestral(const float* __restrict__ x, const float* __restrict__ eps, float cr, float crm1, float c1,
                            float c2, float std, const float* __restrict__ noise, float* __restrict__ out, size_t n) {
    EW_LOOP(i, n) out[i] = ancestral_rn(x[i], eps[i], cr, crm1, c1, c2, std, noise, i);
}
int ancestral_step(const float* x, const float* eps, float sqrt_recip, float sqrt_recipm1, float coef1, float coef2,
                   float std, const float* noise, float* out, size_t n, hipStream_t s) {
    FGDM_LAUNCH(k_ancestral, dim3(ew_grid(n)), dim3(EW_BLOCK), 0, s, x, eps, sqrt_recip, sqrt_recipm1, coef1,
                       coef2, std, noise, out, n);
    return LAUNCH_OK();
}

// One launch per network evaluation of the device ancestral loop (fgdm_sample_ancestral; ddpm.py:1382-1430), one pass over the n
// elements: x' = k_ancestral(x, eps), then THIS step's inpainting blend x = q m + (1 - m) x' with q = sa_t x0 + s1m_t qnoise
// (k_axpby, then k_mask_blend; ddpm.py:1419-1421), then the stores to the state, to the network's input and, on a logged step, to
// the log plane.  p_sample_loop blends AFTER the update, at the timestep of the step that just ran, and logs the blended x; the
// DDIM-family walks (k_loop_step) blend IN FRONT of the next step, at the next timestep, and log x_prev before that blend.  So a
// walk cut into several calls carries nothing over but x.  There is no CFG: p_sample has none.
__global__ void k_ancestral_loop_step(const AncestralLoopStep a) {
    EW_LOOP(i, a.io.n) {
        float xn = ancestral_rn(a.io.x[i], step_eps(a.io, i), a.cr, a.crm1, a.c1, a.c2, a.std, a.noise, i);
        if (!a.noise && a.gen.step_on) xn = add_noise_rn(xn, a.std, noise_step(a.gen, i));
        if (a.mask) xn = mask_blend_rn(axpby_rn(a.sa_t, a.x0[i], a.s1m_t, a.qnoise ? a.qnoise[i] : noise_q(a.gen, i)), xn, a.mask[i]);
        step_store(a.io, i, xn);
        if (a.io.log_x) a.io.log_x[i] = xn;
    }
}
int ancestral_loop_step(const AncestralLoopStep& a, hipStream_t s) {
    if (!step_io_ok(a.io) || (a.mask && (!a.x0 || (!a.qnoise && !a.gen.q_on))) || !noise_gen_ok(a.gen, a.io.n)) return FGDM_ERR_ARG;
    AncestralLoopStep b = a;
    // std == 0 is the t == 0 step: the per-step route hands k_ancestral no noise there.  (With temperature 0 std is 0 at t > 0 too,
    // where that route computes fma(0, noise, mean): a difference only in the sign of an exact zero, or on non-finite noise.)
    if (b.std == 0.f) { b.noise = nullptr; b.gen.step_on = 0; }
    FGDM_LAUNCH(k_ancestral_loop_step, dim3(ew_grid(b.io.n)), dim3(EW_BLOCK), 0, s, b);
    return LAUNCH_OK();
}

// One launch per network evaluation of the device DDIM inversion (fgdm_ddim_encode; ddim_hacked.py:234-279):
// e = CFG(ec, eu) as k_ddim_step's e_out, x_next = k_axpby(x, cx, e, ce), stored to the state, to both halves of the network's
// input and, on a logged step, to the log plane.
__global__ void k_invert_loop_step(const InvertLoopStep a) {
    EW_LOOP(i, a.io.n) {
        const float xn = axpby_rn(a.cx, a.io.x[i], a.ce, step_eps(a.io, i));
        step_store(a.io, i, xn);
        if (a.io.log_x) a.io.log_x[i] = xn;
    }
}
int invert_loop_step(const InvertLoopStep& a, hipStream_t s) {
    if (!step_io_ok(a.io)) return FGDM_ERR_ARG;
    FGDM_LAUNCH(k_invert_loop_step, dim3(ew_grid(a.io.n)), dim3(EW_BLOCK), 0, s, a);
    return LAUNCH_OK();
}

// The generator of the armed loops on its own (noise.h): fgdm_randn's plane, which an unarmed loop and the per-step route read, and
// the raw words of fgdm_op_rand_bits.
__global__ void k_randn_fill(uint32_t key0, uint32_t key1, uint32_t stream_id, uint32_t step, uint32_t first_sample, int repeat,
                             float temperature, uint32_t per_sample, float* __restrict__ out, size_t n) {
    EW_LOOP(i, n) out[i] = noise_normal(key0, key1, stream_id, step, first_sample, repeat, temperature, per_sample, i);
}
int randn_fill(uint64_t seed, uint32_t stream_id, uint32_t step, uint32_t first_sample, int repeat, float temperature, float* out,
               int B, uint32_t per_sample, hipStream_t s) {
    if (!out || B <= 0 || per_sample == 0 || per_sample % 4 != 0) return FGDM_ERR_ARG;
    const size_t n = (size_t)B * per_sample;
    FGDM_LAUNCH(k_randn_fill, dim3(ew_grid(n)), dim3(EW_BLOCK), 0, s, (uint32_t)seed, (uint32_t)(seed >> 32), stream_id, step,
                first_sample, repeat, temperature, per_sample, out, n);
    return LAUNCH_OK();
}
__global__ void k_rand_bits(uint32_t key0, uint32_t key1, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                            uint32_t* __restrict__ out, size_t n_blocks) {
    EW_LOOP(k, n_blocks) {
        const uint64_t lo = ((uint64_t)c1 << 32 | c0) + k, hi = ((uint64_t)c3 << 32 | c2) + (lo < k ? 1u : 0u);
        const PhiloxWords w = philox4x32_10((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32), key0, key1);
#pragma unroll
        for (int j = 0; j < 4; ++j) out[4 * k + j] = w.r[j];
    }
}
int rand_bits(uint64_t seed, const uint32_t c[4], uint32_t* out, size_t n_blocks, hipStream_t s) {
    if (!c || !out || n_blocks == 0) return FGDM_ERR_ARG;
    FGDM_LAUNCH(k_rand_bits, dim3(ew_grid(n_blocks)), dim3(EW_BLOCK), 0, s, (uint32_t)seed, (uint32_t)(seed >> 32), c[0], c[1], c[2],
                c[3], out, n_blocks);
    return LAUNCH_OK();
}

// ---------------------------------------------------------------- first-stage decoder helpers
// post_quant_conv (1x1, 4 -> 4; ldm/models/autoencoder.py:331) applied to scale * z, fused with the layout change:
// z [B, 4, HW] fp32  ->  y [B, HW, 4] fp16.   wb = 16 weights [co][ci] then 4 biases (device, fp32)
__global__ void k_vae_prequant(const float* __restrict__ z, const float* __restrict__ wb, float scale,
                               half_t* __restrict__ y, int B, int HW) {
    const size_t n = (size_t)B * HW;
    EW_LOOP(i, n) {
        const size_t b = i / HW, p = i - b * HW;
        float v[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = scale * z[(b * 4 + c) * HW + p];
        h4 o;
#pragma unroll
        for (int co = 0; co < 4; ++co) {
            float acc = wb[16 + co];
#pragma unroll
            for (int ci = 0; ci < 4; ++ci) acc += wb[co * 4 + ci] * v[ci];
            o[co] = (half_t)acc;
        }
        *(h4*)(y + i * 4) = o;
    }
}
int vae_prequant(const float* z, const float* wb, float scale, half_t* y, int B, int HW, hipStream_t s) {
    FGDM_LAUNCH(k_vae_prequant, dim3(ew_grid((size_t)B * HW)), dim3(EW_BLOCK), 0, s, z, wb, scale, y, B, HW);
    return LAUNCH_OK();
}

// ---------------------------------------------------------------- first-stage encoder helpers
// quant_conv (1x1, 8 -> 8; ldm/models/autoencoder.py:326) applied to the encoder's conv_out, fused with the layout change:
// h [B, HW, 8] fp32 (the GEMM's OUT_F32 rows)  ->  moments [B, 8, HW] fp32.   wb = 64 weights [co][ci] then 8 biases (device, fp32)
__global__ void k_vae_moments(const float* __restrict__ h, const float* __restrict__ wb, float* __restrict__ moments, int B, int HW) {
    const size_t n = (size_t)B * HW;
    EW_LOOP(i, n) {
        const size_t b = i / HW, p = i - b * HW;
        const f32x4 lo = *(const f32x4*)(h + i * 8), hi = *(const f32x4*)(h + i * 8 + 4);
        const float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
        for (int co = 0; co < 8; ++co) {
            float acc = wb[64 + co];
#pragma unroll
            for (int ci = 0; ci < 8; ++ci) acc += wb[co * 8 + ci] * v[ci];
            moments[(b * 8 + co) * HW + p] = acc;
        }
    }
}
int vae_moments(const float* h, const float* wb, float* moments, int B, int HW, hipStream_t s) {
    FGDM_LAUNCH(k_vae_moments, dim3(ew_grid((size_t)B * HW)), dim3(EW_BLOCK), 0, s, h, wb, moments, B, HW);
    return LAUNCH_OK();
}
// (k_posterior_sample, the other first-stage encoder helper, lives in boundary.hip: it must be compiled without contraction)

// P[r][:] = softmax(S[r][:]) over `cols` fp32 logits -> fp16 probabilities; one 256-thread block per row
// (AttnBlock, ldm/modules/diffusionmodules/model.py:190-192: single head, the T x T score matrix of one image)
__global__ __launch_bounds__(256) void k_softmax_rows(const float* __restrict__ S, half_t* __restrict__ P, int cols) {
    __shared__ float red[8];
    const float* row = S + (size_t)blockIdx.x * cols;
    half_t* out = P + (size_t)blockIdx.x * cols;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float m = -INFINITY;
    for (int c = tid; c < cols; c += 256) m = fmaxf(m, row[c]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    if (lane == 0) red[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    float sum = 0.f;
    for (int c = tid; c < cols; c += 256) sum += __expf(row[c] - m);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
    if (lane == 0) red[4 + wave] = sum;
    __syncthreads();
    const float inv = 1.0f / ((red[4] + red[5]) + (red[6] + red[7]));
    for (int c = tid; c < cols; c += 256) out[c] = (half_t)(__expf(row[c] - m) * inv);
}
int softmax_rows(const float* S, half_t* P, int rows, int cols, hipStream_t s) {
    if (rows <= 0 || cols <= 0) return FGDM_ERR_ARG;
    FGDM_LAUNCH(k_softmax_rows, dim3(rows), dim3(256), 0, s, S, P, cols);
    return LAUNCH_OK();
}
