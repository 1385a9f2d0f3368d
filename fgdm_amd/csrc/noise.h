// Counter-based standard normals for the stochastic sampler loops (fgdm_loop_noise_set, fgdm_randn, fgdm_op_rand_bits of
// include/fgdm.h): Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11) and Box-Muller.  Header
// only; every kernel that makes noise calls noise_normal, so the armed loops, fgdm_randn and the per-step route give the same bits.
//
// The normal of element j of sample b at walk position i on stream s is a function of (seed, s, i, global index of b, j) alone:
//   key     = the 64-bit seed, low word first
//   counter = (j >> 2, global sample index, walk position, stream id)
//   the four output words give the four normals of elements 4q .. 4q+3 (q = j >> 2): (r0, r1) -> (rho cos theta, rho sin theta),
//   (r2, r3) likewise, with u1 = ((r >> 8) + 1) 2^-24 in (0, 1], u2 = (r >> 8) 2^-24 in [0, 1), rho = sqrtf(-2 logf(u1)) and
//   theta = 2 pi u2, taken as sincospif(2 u2): 2 u2 is exact in fp32, so the argument carries no rounding of its own.
// u1 >= 2^-24 bounds rho by sqrt(48 ln 2) = 5.7684: |z| <= 5.77 by construction (a normal exceeds that with probability 8e-9).
// logf / sqrtf / sincospif are the accurate forms, not the __-prefixed fast ones.  A thread that handles one element recomputes
// the block of four and keeps one of them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

enum { NOISE_STREAM_STEP = 0, NOISE_STREAM_Q = 1 };      // stream ids: the sampler's step noise, q_sample's noise

struct PhiloxWords { uint32_t r[4]; };

__host__ __device__ __forceinline__ PhiloxWords philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return PhiloxWords{{c0, c1, c2, c3}};
}

// What a kernel needs to make the noise of one launch: the key, where row 0 and the launch sit in the walk, and which of the two
// streams it makes instead of reading a plane (step_on / q_on; a plane that is given wins, the host decides).  Streams keep their
// own walk position: k_loop_step blends in front of the NEXT step.
struct NoiseGen {
    uint32_t key0, key1;
    uint32_t first_sample, per_sample;      // global index of row 0; elements per sample (C H W, a multiple of 4)
    uint32_t step, q_step;                  // walk position of stream 0 / of stream 1 in this launch
    float temperature;                      // stream 0 only: the value used is mul(temperature, z), rounded once
    int repeat;                             // stream 0 only: every row is sample 0 (noise_like(..., repeat=True))
    int step_on, q_on;
};

#ifdef __HIPCC__
__device__ __forceinline__ float noise_mul_rn(float a, float b) {
    float p = a * b;
    asm volatile("" : "+v"(p));             // a value in a register: never the multiplicand of a contracted FMA
    return p;
}
// element `lane` (0..3) of the block of four normals behind the words r
__device__ __forceinline__ float noise_box_muller(const PhiloxWords& w, uint32_t lane) {
    const uint32_t ra = w.r[lane & 2u], rb = w.r[(lane & 2u) + 1u];
    const float u1 = (float)((ra >> 8) + 1u) * 0x1p-24f, u2 = (float)(rb >> 8) * 0x1p-24f;
    const float rho = sqrtf(-2.0f * logf(u1));
    float sn, cs;
    sincospif(2.0f * u2, &sn, &cs);
    return noise_mul_rn(rho, (lane & 1u) ? sn : cs);
}
// the normal of element i of a [B, per_sample] plane: sample = first_sample + i / per_sample (0 where `repeat`), times temperature
__device__ __forceinline__ float noise_normal(uint32_t key0, uint32_t key1, uint32_t stream, uint32_t step, uint32_t first_sample,
                                              int repeat, float temperature, uint32_t per_sample, size_t i) {
    const uint32_t b = (uint32_t)(i / per_sample), j = (uint32_t)(i - (size_t)b * per_sample);
    const PhiloxWords w = philox4x32_10(j >> 2, repeat ? 0u : first_sample + b, step, stream, key0, key1);
    return noise_mul_rn(temperature, noise_box_muller(w, j & 3u));
}
__device__ __forceinline__ float noise_step(const NoiseGen& g, size_t i) {
    return noise_normal(g.key0, g.key1, NOISE_STREAM_STEP, g.step, g.first_sample, g.repeat, g.temperature, g.per_sample, i);
}
__device__ __forceinline__ float noise_q(const NoiseGen& g, size_t i) {
    return noise_normal(g.key0, g.key1, NOISE_STREAM_Q, g.q_step, g.first_sample, 0, 1.0f, g.per_sample, i);
}
#endif
