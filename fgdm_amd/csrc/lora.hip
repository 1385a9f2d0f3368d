// LoRA merge: out[o, i] = W[o, i] + s * sum_{k < r} up[o, k] * down[k, i], all fp32, W taken as [O, I] (a conv weight as
// [Cout, Cin kh kw]).  Runs once per adapter and tensor, never per step: a plain tiled kernel, no MFMA (whose internal summation
// order would make the bits below unpinnable).
#include "common.h"

#define LORA_TO 16          // rows of a tile (each lane walks 4 of them)
#define LORA_TI 64          // columns of a tile: one lane per column, so loads and stores are coalesced along i
#define LORA_RMAX 128

// The arithmetic, written once: the rank sum in ascending k as fmaf into an fp32 accumulator that starts at 0, then one
// fmaf(s, acc, W).  One lane computes one output element from start to end, so the result does not depend on grid or tile.
__device__ __forceinline__ float lora_merge_rn(float w, float s, const float* up_row, const float* down_col, int r) {
    float acc = 0.f;
    for (int k = 0; k < r; ++k) acc = __builtin_fmaf(up_row[k], down_col[k * LORA_TI], acc);
    return __builtin_fmaf(s, acc, w);
}

// block (LORA_TI, 4): up rows [LORA_TO][r] and down columns [r][LORA_TI] of the tile in LDS (8 KB + 32 KB at r = 128)
__global__ void __launch_bounds__(256) k_lora_merge(const float* W, const float* __restrict__ up, const float* __restrict__ down,
                                                    float s, int O, int I, int r, float* out) {
    __shared__ float s_up[LORA_TO * LORA_RMAX];
    __shared__ float s_down[LORA_RMAX * LORA_TI];
    const int tx = threadIdx.x, ty = threadIdx.y, tid = ty * LORA_TI + tx;
    const int o0 = blockIdx.y * LORA_TO, i0 = blockIdx.x * LORA_TI;
    for (int e = tid; e < LORA_TO * r; e += 256) {
        const int o = o0 + e / r;
        s_up[e] = o < O ? up[(size_t)o * r + e % r] : 0.f;
    }
    for (int e = tid; e < r * LORA_TI; e += 256) {
        const int i = i0 + (e & (LORA_TI - 1));
        s_down[e] = i < I ? down[(size_t)(e / LORA_TI) * I + i] : 0.f;
    }
    __syncthreads();
    const int i = i0 + tx;
    if (i >= I) return;
    for (int j = ty; j < LORA_TO; j += 4) {
        const int o = o0 + j;
        if (o >= O) break;
        const size_t at = (size_t)o * I + i;
        out[at] = lora_merge_rn(W[at], s, s_up + j * r, s_down + tx, r);      // read before written by the same lane: out may be W
    }
}

int lora_merge(const float* W, const float* up, const float* down, float s, int O, int I, int r, float* out, hipStream_t st) {
    const int gy = (O + LORA_TO - 1) / LORA_TO;
    if (r < 1 || r > LORA_RMAX || gy > 65535) return FGDM_ERR_ARG;
    FGDM_LAUNCH(k_lora_merge, dim3((I + LORA_TI - 1) / LORA_TI, gy), dim3(LORA_TI, 4), 0, st, W, up, down, s, O, I, r, out);
    return hipGetLastError() == hipSuccess ? FGDM_OK : FGDM_ERR_HIP;
}
