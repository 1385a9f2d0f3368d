// Host helpers shared by engine.hip and the C-ABI files beside it (ops_abi.hip: op-level test entries; bench_abi.hip:
// micro-benchmark entries): the launch sequences the op entries must run exactly as the engine runs them, and the small device
// temporaries of the entries that own their buffers.
#pragma once
#include "common.h"
#include "../../include/fgdm.h"

#include <algorithm>
#include <cmath>
#include <vector>

static int roundup(int x, int m) { return (x + m - 1) / m * m; }

// Column order of a packed conv3x3 weight row: kmap[k_packed] = index into the source row [Cin][3][3], or -1 for a pad column
// (left zero).  Cin % 64 == 0, implicit GEMM: k = (c / 64 * 9 + tap) * 64 + c % 64 (64-channel chunk outermost, then tap: the order
// the kernels walk K, see igemm2.hip), *cin_pad = Cin, K = 9 Cin.  Otherwise the im2col route: channels padded to *cin_pad (a
// multiple of 8 when Cin is one, else of 4: the granule of k_im2col), k = tap * cin_pad + c, K = roundup64(9 cin_pad).
// One function for Engine::pack_conv3 and fgdm_op_conv2d.
static std::vector<int> conv3_kmap(int Cin, int* cin_pad) {
    const bool implicit = (Cin % 64) == 0;
    const int cp = implicit ? Cin : roundup(Cin, Cin % 8 == 0 ? 8 : 4);
    const int K = implicit ? 9 * Cin : roundup(9 * cp, 64);
    std::vector<int> kmap(K, -1);
    for (int tap = 0; tap < 9; ++tap)
        for (int c = 0; c < Cin; ++c) {
            const int k = implicit ? ((c >> 6) * 9 + tap) * 64 + (c & 63) : tap * cp + c;
            kmap[k] = c * 9 + tap;
        }
    *cin_pad = cp;
    return kmap;
}

// Upsample = nearest-2x, then conv3x3 (openaimodel.py: Upsample.forward).  Rows 2 i + a - 1 .. 2 i + a + 1 of the upsampled image are
// source rows {i - 1, i, i} (a = 0) or {i, i, i + 1} (a = 1), columns likewise with b: output phase (a, b) is a 2x2 convolution over
// the source at displacement (a - 1 + ty, b - 1 + tx) whose tap (ty, tx) is the SUM of the 3x3 taps that land on that source pixel
//     a = 0: ty 0 = w[0], ty 1 = w[1] + w[2]        a = 1: ty 0 = w[0] + w[1], ty 1 = w[2]        (columns: b, tx, kx alike)
// and the zero padding of the upsampled image is "source index -1 or H reads zero".  w [N][Cin][3][3] fp32 -> [4 phases][npad][4 Cin]
// fp16, phase = 2 a + b, k = (2 ty + tx) Cin + c; the sums are taken in fp32 (ky-major order) and rounded ONCE.
// One function for Engine::pack_conv3 and fgdm_op_conv2d.
static std::vector<half_t> up_phase_pack(const float* w, int N, int Cin, size_t npad) {
    const size_t K = 4 * (size_t)Cin;
    std::vector<half_t> pk(4 * npad * K, (half_t)0);
    for (int phs = 0; phs < 4; ++phs) {
        const int a = phs >> 1, b = phs & 1;
        for (int n = 0; n < N; ++n)
            for (int c = 0; c < Cin; ++c) {
                const float* src = w + ((size_t)n * Cin + c) * 9;
                for (int t = 0; t < 4; ++t) {
                    const int ty = t >> 1, tx = t & 1;
                    const int ky0 = ty == 0 ? 0 : (a == 0 ? 1 : 2), ky1 = ty == 0 ? (a == 0 ? 0 : 1) : 2;
                    const int kx0 = tx == 0 ? 0 : (b == 0 ? 1 : 2), kx1 = tx == 0 ? (b == 0 ? 0 : 1) : 2;
                    float sum = 0.f;
                    for (int ky = ky0; ky <= ky1; ++ky)
                        for (int kx = kx0; kx <= kx1; ++kx) sum += src[ky * 3 + kx];
                    pk[((size_t)phs * npad + n) * K + (size_t)t * Cin + c] = (half_t)sum;
                }
            }
    }
    return pk;
}

// The im2col route of a conv3x3 (padding 1, stride 1 or 2): A[m][tap * C + c] into the caller's workspace A [B Ho Wo, K], then
// `gemm_rows(A, B, Ho, Wo, K, rows_per_sample)`: the caller's LINEAR GEMM over the rows of A viewed as [B, Ho, Wo, K], the rows
// of one sample being its Ho Wo output pixels.  One sequence for Engine::conv3 (whose GEMM goes through the engine's arena and
// timer) and fgdm_op_conv2d (caller-owned buffers); `after_im2col()` closes the engine's timer bracket around the first kernel.
template <class After, class Gemm>
static int im2col_conv(const half_t* x, half_t* A, int B, int H, int W, int C, int stride, int K, hipStream_t s,
                       After&& after_im2col, Gemm&& gemm_rows) {
    const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    const int rc = im2col3x3(x, A, B, H, W, C, stride, K, s);
    after_im2col();
    if (rc != FGDM_OK) return rc;
    return gemm_rows(A, B, Ho, Wo, K, Ho * Wo);
}

// The core of AttnBlock.forward (model.py:188-199) for B images of T tokens, ONE head over all C channels, per image:
// S = C^-1/2 Q K^T (fp32 [T, T]; a GEMM whose "weight" is the image's K rows), P = row softmax (fp16), O = P V (a GEMM over
// K = T whose weight is the image's V^T [C, T]).  S and P are reused by every image.  q [B T, C]; k [B T + 128, C] (the GEMM
// reads whole weight tiles of up to 128 rows: the rows after an image's keys must be readable and finite, they feed only score
// columns >= T that are never written); vt [B, C, T]; out [B T, C].
// `gemm_rows(Wt, N, K, A, M, out_kind, out, ld_out, scale)`: the caller's LINEAR GEMM out = scale * A Wt^T without bias.
// One loop for Engine::vattn_fwd and fgdm_op_vae_attention.  Returns the first failing step's code; *softmax_failed tells which.
template <class Gemm>
static int vattn_core(const half_t* q, const half_t* k, const half_t* vt, half_t* out, float* S, half_t* P, int B, int T, int C,
                      hipStream_t s, bool* softmax_failed, Gemm&& gemm_rows) {
    *softmax_failed = false;
    for (int b = 0; b < B; ++b) {
        int rc = gemm_rows(k + (size_t)b * T * C, T, C, q + (size_t)b * T * C, T, OUT_F32, (void*)S, T, 1.0f / sqrtf((float)C));
        if (rc != FGDM_OK) return rc;
        if (softmax_rows(S, P, T, T, s) != FGDM_OK) { *softmax_failed = true; return FGDM_ERR_HIP; }
        rc = gemm_rows(vt + (size_t)b * C * T, C, T, P, T, OUT_F16, (void*)(out + (size_t)b * T * C), C, 1.0f);
        if (rc != FGDM_OK) return rc;
    }
    return FGDM_OK;
}

static hipStream_t as_stream(void* p) { return (hipStream_t)p; }

// Device temporaries of one op-level / benchmark call: freed when it returns (synchronise first)
struct TmpDev {
    std::vector<void*> ptrs;
    ~TmpDev() { for (void* p : ptrs) (void)hipFree(p); }
    template <typename T> T* alloc(size_t n) {
        T* d = nullptr;
        if (hipMalloc(&d, n * sizeof(T)) != hipSuccess) return nullptr;
        ptrs.push_back(d);
        return d;
    }
    template <typename T> T* up(const std::vector<T>& h) {
        T* d = alloc<T>(std::max<size_t>(h.size(), 256 / sizeof(T)));
        if (d) (void)hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
        return d;
    }
};
// the split-K plan the engine would make for `a` (operands and epilogue filled in), with its workspace from `tmp`
static int plan_splitk(IgemmArgs& a, TmpDev& tmp) {
    a.splitk = igemm_splitk_factor(a);
    if (a.splitk > 1 && !(a.ws = tmp.alloc<float>((size_t)a.splitk * a.M * a.N))) return FGDM_ERR_NOMEM;
    return FGDM_OK;
}
inline half_t* g_zero_page() {       // one page for the whole library
    static half_t* z = nullptr;
    if (!z) { if (hipMalloc(&z, 4096) != hipSuccess) return nullptr; (void)hipMemset(z, 0, 4096); }
    return z;
}
