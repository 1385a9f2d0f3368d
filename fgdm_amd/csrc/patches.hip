// Patch-wise evaluation of large images (the reference's `split_input_params` routes, ldm/models/diffusion/ddpm.py:713-763,
// 841-878, 1046-1128): cut an NCHW fp32 tensor into overlapping crops (torch.nn.Unfold), and blend the networks' results on
// the crops back into one tensor (torch.nn.Fold of crop * weighting, divided by the folded weighting).  HBM-bound gathers:
// one thread per group of V = 4 (16-byte accesses, when widths, strides and pointers allow) or 1 contiguous elements; every
// output element is computed by exactly one thread, in a fixed order, so no atomics and no dependence on the pass size.
// Built with -ffp-contract=off (build.py): w * o is rounded before it is added, as the reference's separate multiply and fold.
#include "common.h"
#include "../../include/fgdm.h"

#include <algorithm>

#define PT_BLOCK 256
static inline int pt_grid(size_t n) {
    size_t g = (n + PT_BLOCK - 1) / PT_BLOCK;
    return (int)(g > 8192 ? 8192 : (g < 1 ? 1 : g));
}
#define PT_LOOP(i, n) for (size_t i = (size_t)blockIdx.x * PT_BLOCK + threadIdx.x; i < (n); i += (size_t)gridDim.x * PT_BLOCK)
#define LAUNCH_OK() (hipGetLastError() == hipSuccess ? FGDM_OK : FGDM_ERR_HIP)

template <int V> struct PVec { typedef float t __attribute__((ext_vector_type(V))); };
template <> struct PVec<1> { typedef float t; };

// Crops l = ly * Lx + lx of [kh, kw] cells with the top-left corner at (ly * sh, lx * sw): the column order of torch.nn.Unfold
int patch_plan(int H, int W, int kh, int kw, int sh, int sw, bool must_cover, int* Ly, int* Lx) {
    if (H <= 0 || W <= 0 || kh <= 0 || kw <= 0 || sh <= 0 || sw <= 0 || kh > H || kw > W) return FGDM_ERR_ARG;
    if (must_cover && (sh > kh || sw > kw || (H - kh) % sh || (W - kw) % sw)) return FGDM_ERR_ARG;
    *Ly = (H - kh) / sh + 1;
    *Lx = (W - kw) / sw + 1;
    return FGDM_OK;
}

// x [B, C, H, W] -> out [n, B, C, kh, kw]: crops [l0, l0 + n)
template <int V>
__global__ void k_unfold(const float* __restrict__ x, float* __restrict__ out, PatchGeom g, int l0, int n) {
    typedef typename PVec<V>::t vec_t;
    const int kwg = g.kw / V;
    const size_t BC = (size_t)g.B * g.C;
    const size_t total = (size_t)n * BC * g.kh * kwg;
    PT_LOOP(i, total) {
        const int kx = (int)(i % kwg) * V;
        size_t r = i / kwg;
        const int ky = (int)(r % g.kh);
        r /= g.kh;
        const size_t bc = r % BC;
        const int l = l0 + (int)(r / BC);
        const int y0 = (l / g.Lx) * g.sh, x0 = (l % g.Lx) * g.sw;
        *(vec_t*)(out + i * V) = *(const vec_t*)(x + (bc * g.H + y0 + ky) * g.W + x0 + kx);
    }
}

// first and last crop index along one axis whose [i * s, i * s + k) holds coordinate p
__device__ __forceinline__ void covering(int p, int k, int s, int L, int* lo, int* hi) {
    *lo = p < k ? 0 : (p - k) / s + 1;
    *hi = min(L - 1, p / s);
}

// acc [B, C, H, W] (+)= sum over the crops l in [l0, l0 + n) that cover the pixel, ascending l, of
// (w_pix[ky, kx] * w_tie[l]) * o[l - l0, b, c, ky, kx].  l0 == 0 starts from zero (acc needs no memset); later passes continue the
// same running sum, so the additions of a pixel happen in the same order whatever the pass size.  The V pixels of a thread
// share their covering crops (V == 4 only when W, kw and sw are multiples of 4).
template <int V>
__global__ void k_fold_accumulate(const float* __restrict__ o, const float* __restrict__ w_pix, const float* __restrict__ w_tie,
                                  float* __restrict__ acc, PatchGeom g, int l0, int n) {
    typedef typename PVec<V>::t vec_t;
    const int wg = g.W / V;
    const size_t BC = (size_t)g.B * g.C;
    const size_t total = BC * g.H * wg;
    PT_LOOP(i, total) {
        const int x = (int)(i % wg) * V;
        const size_t r = i / wg;
        const int y = (int)(r % g.H);
        const size_t bc = r / g.H;
        int ly0, ly1, lx0, lx1;
        covering(y, g.kh, g.sh, g.Ly, &ly0, &ly1);
        covering(x, g.kw, g.sw, g.Lx, &lx0, &lx1);
        vec_t s = l0 == 0 ? (vec_t)0.0f : *(const vec_t*)(acc + i * V);
        for (int ly = ly0; ly <= ly1; ++ly)
            for (int lx = lx0; lx <= lx1; ++lx) {
                const int l = ly * g.Lx + lx;
                if (l < l0 || l >= l0 + n) continue;
                const int ky = y - ly * g.sh, kx = x - lx * g.sw;
                const vec_t w = *(const vec_t*)(w_pix + ky * g.kw + kx) * w_tie[l];
                const vec_t v = *(const vec_t*)(o + ((((size_t)(l - l0) * BC + bc) * g.kh + ky) * g.kw + kx));
                s += w * v;
            }
        *(vec_t*)(acc + i * V) = s;
    }
}

// out = acc / norm, norm[y, x] = sum over ALL covering crops, ascending l, of w_pix * w_tie (the folded weighting, recomputed per
// pixel: at most a handful of terms).  out may be acc.
template <int V>
__global__ void k_fold_finish(const float* acc, const float* __restrict__ w_pix, const float* __restrict__ w_tie, float* out,
                              PatchGeom g) {
    typedef typename PVec<V>::t vec_t;
    const int wg = g.W / V;
    const size_t total = (size_t)g.B * g.C * g.H * wg;
    PT_LOOP(i, total) {
        const int x = (int)(i % wg) * V;
        const int y = (int)((i / wg) % g.H);
        int ly0, ly1, lx0, lx1;
        covering(y, g.kh, g.sh, g.Ly, &ly0, &ly1);
        covering(x, g.kw, g.sw, g.Lx, &lx0, &lx1);
        vec_t norm = (vec_t)0.0f;
        for (int ly = ly0; ly <= ly1; ++ly)
            for (int lx = lx0; lx <= lx1; ++lx)
                norm += *(const vec_t*)(w_pix + (y - ly * g.sh) * g.kw + (x - lx * g.sw)) * w_tie[ly * g.Lx + lx];
        *(vec_t*)(out + i * V) = *(const vec_t*)(acc + i * V) / norm;
    }
}

// dst [reps][words] = src [words] repeated (32-bit words): the timesteps and the context of every crop of a pass
__global__ void k_repeat(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, size_t words, int reps) {
    PT_LOOP(i, words * (size_t)reps) dst[i] = src[i % words];
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static bool wide(const PatchGeom& g) { return g.W % 4 == 0 && g.kw % 4 == 0 && g.sw % 4 == 0; }
static bool geom_ok(const PatchGeom& g, int l0, int n) {
    return g.B > 0 && g.C > 0 && g.Ly > 0 && g.Lx > 0 && l0 >= 0 && n > 0 && (long long)l0 + n <= (long long)g.Ly * g.Lx;
}

int unfold_crops(const float* x, float* out, const PatchGeom& g, int l0, int n, hipStream_t s) {
    if (!geom_ok(g, l0, n)) return FGDM_ERR_ARG;
    const size_t total = (size_t)n * g.B * g.C * g.kh * g.kw;
    if (wide(g) && aligned16(x) && aligned16(out))
        FGDM_LAUNCH(k_unfold<4>, dim3(pt_grid(total / 4)), dim3(PT_BLOCK), 0, s, x, out, g, l0, n);
    else
        FGDM_LAUNCH(k_unfold<1>, dim3(pt_grid(total)), dim3(PT_BLOCK), 0, s, x, out, g, l0, n);
    return LAUNCH_OK();
}

int fold_accumulate(const float* o, const float* w_pix, const float* w_tie, float* acc, const PatchGeom& g, int l0, int n,
                    hipStream_t s) {
    if (!geom_ok(g, l0, n)) return FGDM_ERR_ARG;
    const size_t total = (size_t)g.B * g.C * g.H * g.W;
    if (wide(g) && aligned16(o) && aligned16(w_pix) && aligned16(acc))
        FGDM_LAUNCH(k_fold_accumulate<4>, dim3(pt_grid(total / 4)), dim3(PT_BLOCK), 0, s, o, w_pix, w_tie, acc, g, l0, n);
    else
        FGDM_LAUNCH(k_fold_accumulate<1>, dim3(pt_grid(total)), dim3(PT_BLOCK), 0, s, o, w_pix, w_tie, acc, g, l0, n);
    return LAUNCH_OK();
}

int fold_finish(const float* acc, const float* w_pix, const float* w_tie, float* out, const PatchGeom& g, hipStream_t s) {
    if (!geom_ok(g, 0, 1)) return FGDM_ERR_ARG;
    const size_t total = (size_t)g.B * g.C * g.H * g.W;
    if (wide(g) && aligned16(acc) && aligned16(w_pix) && aligned16(out))
        FGDM_LAUNCH(k_fold_finish<4>, dim3(pt_grid(total / 4)), dim3(PT_BLOCK), 0, s, acc, w_pix, w_tie, out, g);
    else
        FGDM_LAUNCH(k_fold_finish<1>, dim3(pt_grid(total)), dim3(PT_BLOCK), 0, s, acc, w_pix, w_tie, out, g);
    return LAUNCH_OK();
}

int repeat_words(const void* src, void* dst, size_t words, int reps, hipStream_t s) {
    if (words == 0 || reps <= 0) return FGDM_ERR_ARG;
    FGDM_LAUNCH(k_repeat, dim3(pt_grid(words * (size_t)reps)), dim3(PT_BLOCK), 0, s, (const uint32_t*)src, (uint32_t*)dst, words, reps);
    return LAUNCH_OK();
}

// ------------------------------------------------------------------------------------------------ stateless C ABI
extern "C" {

int fgdm_unfold(const float* x, int B, int C, int H, int W, int kh, int kw, int sh, int sw, int l0, int n, float* crops,
                void* stream) {
    if (!x || !crops) return FGDM_ERR_ARG;
    PatchGeom g{B, C, H, W, kh, kw, sh, sw, 0, 0};
    if (patch_plan(H, W, kh, kw, sh, sw, false, &g.Ly, &g.Lx) != FGDM_OK) return FGDM_ERR_ARG;
    return unfold_crops(x, crops, g, l0, n, (hipStream_t)stream);
}

int fgdm_fold_weighted(const float* crops, const float* w_pix, const float* w_tie, int B, int C, int Ho, int Wo, int kh, int kw,
                       int sh, int sw, int crops_per_pass, float* out, void* stream) {
    if (!crops || !w_pix || !w_tie || !out || crops_per_pass < 0) return FGDM_ERR_ARG;
    PatchGeom g{B, C, Ho, Wo, kh, kw, sh, sw, 0, 0};
    if (patch_plan(Ho, Wo, kh, kw, sh, sw, true, &g.Ly, &g.Lx) != FGDM_OK || !geom_ok(g, 0, 1)) return FGDM_ERR_ARG;
    const int L = g.Ly * g.Lx, step = crops_per_pass > 0 ? std::min(crops_per_pass, L) : L;
    const size_t per_crop = (size_t)B * C * kh * kw;
    for (int l0 = 0; l0 < L; l0 += step) {
        const int rc = fold_accumulate(crops + (size_t)l0 * per_crop, w_pix, w_tie, out, g, l0, std::min(step, L - l0), (hipStream_t)stream);
        if (rc != FGDM_OK) return rc;
    }
    return fold_finish(out, w_pix, w_tie, out, g, (hipStream_t)stream);
}

}  // extern "C"
