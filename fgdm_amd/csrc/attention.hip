// Fused (flash-style) multi-head attention for gfx950: O = softmax(Q K^T d^-1/2) V, never materialising scores.
// Reference semantics: CrossAttention.forward, ldm/modules/attention.py:177-202 (self: context = x; cross: 77 tokens).
//
// Layout: Q [B, T, ldq], K [B, Tk, ldk] with head h at columns [h*D, (h+1)*D); V is consumed TRANSPOSED,
// Vt [B, H*D, ldvt] (keys contiguous), which the V-projection GEMM writes directly (OUT_F16_T epilogue).
//
// One workgroup = 4 waves = 128 queries of one (batch, head); each wave owns 32 queries.
//   S^T = K Q^T   : v_mfma_f32_32x32x16_f16 with A = K tile rows (keys), B = Q^T kept in registers, so each lane
//                   holds one query column -> the softmax row reduction is in-lane + one cross-half shuffle.
//   O^T += Vt P^T : the S^T accumulator registers, converted to fp16, ARE the B operand (k order permuted as
//                   16s + 8(j>>2) + 4h + (j&3)); the A operand reads Vt from LDS with the same key permutation.
// The softmax is VALU-bound at d = 40 (one v_exp per score against 14 MFMAs per 64 keys), so the VALU work is cut:
//   * the row sum l = sum_k p rides on the MFMA: the spare rows of the padded O^T tile (d = 40 -> 64, 80 -> 96)
//     get a row of ONES in the Vt LDS tile, so O^T[row D] accumulates sum_k fp16(p) -- exactly the normaliser of
//     the fp16 probabilities used in the numerator -- and is rescaled together with O for free;
//   * deferred-max rescale: the running max is only raised (and O rescaled) when some query of the wave exceeds it
//     by more than 2^8; p <= 256 stays exact-range in fp16 and the final division by l cancels the offset;
//   * K / Vt tiles are double-buffered in LDS and prefetched into registers one tile ahead (one barrier per tile);
//   * d = 40 (padded to 48 in the contraction) has spare k slots: Q is pre-multiplied by log2(e) d^-1/2 and slot 40
//     carries K = 1, Q = -m (the running max, kept fp16-representable), so the MFMA itself delivers
//     s log2(e) d^-1/2 - m and the per-score work shrinks to max3 + exp2 + pack (FOLD).
//
// (variants that were measured and rejected, and what bounds these kernels: DESIGN.md section 4.2 / 4.3)
#include "common.h"
#include "knobs.h"
#include <type_traits>
#include <algorithm>

#pragma clang diagnostic ignored "-Winline-asm"     // M0 named as an asm clobber (att_dma16): reserved register, on purpose
#define ATT_THR 8.0f
#define ATT_SB() __builtin_amdgcn_sched_barrier(0)

// XCD-aware mapping: workgroups b and b+8 share an XCD (and its 4 MiB L2).  Give every XCD a contiguous range of logical blocks, which
// the kernels decode as (batch, head, q-block) triples with the q-block fastest, so all q-blocks of one (batch, head) stream the SAME
// K / Vt through ONE L2 instead of eight (PMC: 389 MB fetched per launch against 252 MB of Q+K+V before).
__device__ __forceinline__ int att_logical_block() {
    const int nb = gridDim.x, bid = blockIdx.x, xcd = bid & 7, qd = nb >> 3, r = nb & 7;
    return (xcd < r ? xcd * (qd + 1) : r * (qd + 1) + (xcd - r) * qd) + (bid >> 3);
}
// Maximum of mx over the two lane halves (the other key half of the same query: lane ^ 32).
// Inline asm, not __builtin_amdgcn_permlane32_swap: hipcc folds fmaxf(r[0], r[1]) of the builtin's two results into r[0] (visible in the
// IR; round 3 met the same fold) and the cross-half maximum silently disappears.  s_nop 1 = the two wait states between a vector-ALU
// write of an operand and the swap that reads it
__device__ __forceinline__ float att_max_cross(float mx) {
    float lo = mx, hi = mx;
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(lo), "+v"(hi));
    return fmaxf(lo, hi);
}

// Capturing instantiations (cross-attention maps, DESIGN.md "Cross-attention maps"): the two kernels that take text contexts carry a
// parameter pack Cap, empty in the instantiations of the product path -- whose signature, registers and instructions are what they
// were -- and one float* in the capturing ones: the per-head probability planes P [B, H, T, Tk] fp32 (row stride exactly Tk: pad
// keys have no slot to be stored in).  P[b, h, t, k] = softmax_k(q k^T d^-1/2), from the fp32 exponentials BEFORE they are rounded to
// fp16 for V^T P^T, divided by their own fp32 sum (not by the fp16 sum that normalises O).  attn_maps_reduce_kernel below averages
// the planes over heads in head order.  Plain per-lane stores; nothing else in the kernel reads them, O keeps its bits.
__device__ __forceinline__ float* att_cap_plane() { return nullptr; }
__device__ __forceinline__ float* att_cap_plane(float* p) { return p; }
#define ATT_CAP_MAX_KEYS 256      // the capturing kernels' key limit (fgdm.h: FGDM_ATTENTION_CAPTURE_MAX_KEYS)

template <int D, class... Cap>
__global__ __launch_bounds__(256) void attn_kernel(const half_t* __restrict__ Q, int ldq,
                                                   const half_t* __restrict__ K, int ldk,
                                                   const half_t* __restrict__ Vt, int ldvt,
                                                   half_t* __restrict__ O, int ldo,
                                                   int H, int T, int Tk, float sl2e, Cap... cap) {
    constexpr bool CAP = sizeof...(Cap) > 0;
    constexpr int DP = (D + 15) / 16 * 16;   // QK^T contraction length, padded to MFMA K
    constexpr int NKS = DP / 16;
    constexpr int DT = (D + 31) / 32;         // 32-row tiles of O^T
    constexpr bool ONES = (DT * 32 > D);      // a spare O^T row exists: row D carries the softmax denominator
    constexpr bool FOLD = (DP > D) && (D % 8 == 0);   // a spare contraction slot exists: scale and -max ride on the MFMA
    constexpr int PS = D / 16, PH = (D % 16) / 8;     // fragment / lane half that hold contraction slot D (element 0)
    constexpr int KS = DP * 2 + 16;           // K-tile row stride in bytes: odd multiple of 16 -> b128 conflict-free
    constexpr int VS = 64 * 2 + 8;            // Vt-tile row stride in bytes: 34 dwords -> b64 conflict-free
    constexpr int DC = D / 8;                 // 16-byte chunks per K row
    constexpr int KCH = (64 * DC + 255) / 256;   // K chunks per thread per tile
    constexpr int VCH = (D * 8 + 255) / 256;     // Vt chunks per thread per tile
    constexpr int KBYTES = 64 * KS, VBYTES = DT * 32 * VS;
    __shared__ __attribute__((aligned(16))) char smem[2 * (KBYTES + VBYTES)];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lq = lane & 31, lh = lane >> 5;
    const int nqb = (T + 127) / 128;
    const int logical = att_logical_block();
    // Cross-attention (Tk <= 128: K / Vt of a head are 6-25 KB, nothing to share) is bound by its Q reads and O writes, and a
    // head's slice of a token row is 2 D bytes of a 2 H D-byte row: there the HEAD runs fastest, so the H workgroups that touch
    // the same 128 rows are neighbours on one XCD and every 128-byte line of Q and O crosses the fabric once instead of once per
    // head that owns a piece of it (only Tk <= 64 still comes here with few keys; the text tokens have attn_cross_kernel below)
    int qblk, b, head;
    if (Tk <= 128) {
        head = logical % H;
        const int rest = logical / H;
        qblk = rest % nqb; b = rest / nqb;
    } else {
        qblk = logical % nqb;
        const int bh = logical / nqb;
        b = bh / H; head = bh - b * H;
    }
    const int q = qblk * 128 + wave * 32 + lq;

    // pad regions of both buffers, written once: K pad columns [D, DP) = 0; Vt pad rows [D, DT*32) = 0, row D = 1
    for (int buf = 0; buf < 2; ++buf) {
        char* Ksb = smem + buf * (KBYTES + VBYTES);
        char* Vsb = Ksb + KBYTES;
        if constexpr (DP > D) {
            for (int i = tid; i < 64 * (DP - D) / 8; i += 256) {
                const int key = i / ((DP - D) / 8), c = i % ((DP - D) / 8);
                h8 pad = (h8)(half_t)0;
                if (FOLD && c == 0) pad[0] = (half_t)1;      // K[key][D] = 1: multiplies the -max kept in Q[q][D]
                *(h8*)(Ksb + key * KS + (D + c * 8) * 2) = pad;
            }
        }
        for (int i = tid; i < (DT * 32 - D) * 16; i += 256) {
            const int r = D + i / 16, c = i % 16;
            *(h4*)(Vsb + r * VS + c * 8) = (r == D) ? (h4)(half_t)1 : (h4)(half_t)0;
        }
    }

    // Q^T fragments (B operand): lane holds Q[q][16s + 8h .. +7]
    h8 qf[NKS];
#pragma unroll
    for (int s = 0; s < NKS; ++s) {
        const int c = 16 * s + 8 * lh;
        qf[s] = (h8)(half_t)0;
        if (c < D && q < T) qf[s] = *(const h8*)(Q + ((size_t)b * T + q) * ldq + head * D + c);
        if constexpr (FOLD) {
#pragma unroll
            for (int j = 0; j < 8; ++j) qf[s][j] = (half_t)((float)qf[s][j] * sl2e);
        }
    }

    f32x16 oacc[DT];
#pragma unroll
    for (int t = 0; t < DT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[t][r] = 0.f;
    float m_run = FOLD ? 0.f : -INFINITY, l_run = 0.f;   // l_run only used when there is no spare row (D = 160)
    // CAP (Tk <= ATT_CAP_MAX_KEYS = four tiles): the softmax is online, so a tile's probabilities are stored as they are -- relative to
    // the running maximum of their tile, cap_m[tile] -- and put right behind the loop, when the final maximum and the fp32 sum cap_l
    // (rescaled with O) are known: each lane multiplies what it stored itself by exp2(cap_m[tile] - m_run) / cap_l
    float cap_l = 0.f, cap_m[CAP ? ATT_CAP_MAX_KEYS / 64 : 1];
    float* cap_row = nullptr;
    if constexpr (CAP) {
#pragma unroll
        for (int j = 0; j < ATT_CAP_MAX_KEYS / 64; ++j) cap_m[j] = 0.f;
        cap_row = att_cap_plane(cap...) + (((size_t)b * H + head) * T + min(q, T - 1)) * Tk;
    }

    const half_t* Kb = K + (size_t)b * Tk * ldk + head * D;
    const half_t* Vb = Vt + ((size_t)b * H + head) * D * ldvt;

    // register prefetch of one K / Vt tile.  Everything per-thread about the copy is loop-invariant and computed here, the
    // tile base is wave-uniform (scalar), chunk validity is wave-uniform too (64 * DC and D * 8 are multiples of 64), and
    // the K loop below is unrolled over the two LDS buffers so that their offsets are immediates: the loop carries no
    // address arithmetic or per-lane predicates (PMC, round 2: 114 VALU instructions per 64-key tile of which 64 were the
    // softmax itself; the kernel is vector-issue bound, so the other 50 cost as much as a fifth of the tile).
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    int k_goff[KCH], k_loff[KCH], k_key[KCH], v_goff[VCH], v_loff[VCH];
#pragma unroll
    for (int u = 0; u < KCH; ++u) {
        const int i = tid + u * 256, key = i / DC, c = i - key * DC;
        k_key[u] = key; k_goff[u] = key * ldk + c * 8; k_loff[u] = key * KS + c * 16;
    }
#pragma unroll
    for (int u = 0; u < VCH; ++u) {
        const int i = tid + u * 256, r = i >> 3, c = i & 7;
        v_goff[u] = r * ldvt + c * 8; v_loff[u] = r * VS + c * 16;
    }
    h8 kreg[KCH], vreg[VCH];
    auto load_tile = [&](int k0, bool ragged) {
        const half_t* kb = Kb + (size_t)k0 * ldk;
        const half_t* vb = Vb + k0;
#pragma unroll
        for (int u = 0; u < KCH; ++u)
            if ((u * 4 + wave_u) * 64 < 64 * DC) {
                int off = k_goff[u];
                // rows past Tk: re-read the last valid row (their scores are masked to -inf below; never out of bounds)
                if (ragged) off += (min(k_key[u], Tk - 1 - k0) - k_key[u]) * ldk;
                kreg[u] = *(const h8*)(kb + off);
            }
#pragma unroll
        for (int u = 0; u < VCH; ++u)
            if ((u * 4 + wave_u) * 64 < D * 8) vreg[u] = *(const h8*)(vb + v_goff[u]);     // Vt rows are padded to 64 keys
    };
    auto store_tile = [&](auto bufc) {
        constexpr int buf = decltype(bufc)::value;
        char* Ksb = smem + buf * (KBYTES + VBYTES);
        char* Vsb = Ksb + KBYTES;
#pragma unroll
        for (int u = 0; u < KCH; ++u)
            if ((u * 4 + wave_u) * 64 < 64 * DC) *(h8*)(Ksb + k_loff[u]) = kreg[u];
#pragma unroll
        for (int u = 0; u < VCH; ++u)
            if ((u * 4 + wave_u) * 64 < D * 8) {
                const h8 v = vreg[u];
                h4 lo = {v[0], v[1], v[2], v[3]}, hi = {v[4], v[5], v[6], v[7]};
                *(h4*)(Vsb + v_loff[u]) = lo;
                *(h4*)(Vsb + v_loff[u] + 8) = hi;
            }
    };
    // fragment addresses inside a tile (bytes): loop-invariant too
    const int kfrag = lq * KS + 8 * lh * 2, vfrag = lq * VS + 4 * lh * 2;

    load_tile(0, Tk < 64);
    store_tile(std::integral_constant<int, 0>{});
    // NSUB = 1: the tile's second 32-key sub-tile lies entirely beyond Tk (cross-attention: 77 keys = 64 + 13) and is skipped --
    // its QK^T and PV MFMAs, its 16 exponentials per lane, its fragment reads
    auto tile = [&](int k0, auto curc, auto nsubc) {
        constexpr int cur = decltype(curc)::value;
        constexpr int NSUB = decltype(nsubc)::value;
        const bool more = k0 + 64 < Tk;
        if (more) load_tile(k0 + 64, k0 + 128 > Tk);      // global loads fly while this tile is computed
        __syncthreads();                   // buffer `cur` is complete; buffer cur^1 is no longer read by anyone
        const char* Ks = smem + cur * (KBYTES + VBYTES);
        const char* Vs = Ks + KBYTES;

        // ---- S^T = K Q^T for two 32-key sub-tiles.  ALL K fragments of the tile are requested first, then the MFMAs run
        // behind counted lgkmcnt waits: a read-wait-MFMA chain per fragment left the wave parked on LDS latency ~13 times per
        // tile (the ISA of the previous version: ds_read_b128, s_waitcnt lgkmcnt(0), v_mfma ... six times over).
        h8 kf[2][NKS];
#pragma unroll
        for (int sub = 0; sub < NSUB; ++sub)
#pragma unroll
            for (int s = 0; s < NKS; ++s) kf[sub][s] = *(const h8*)(Ks + kfrag + sub * 32 * KS + 16 * s * 2);
        __builtin_amdgcn_sched_barrier(0);
        f32x16 sacc[2];
#pragma unroll
        for (int sub = 0; sub < NSUB; ++sub) {
#pragma unroll
            for (int r = 0; r < 16; ++r) sacc[sub][r] = 0.f;
#pragma unroll
            for (int s = 0; s < NKS; ++s) sacc[sub] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[sub][s], qf[s], sacc[sub], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        // ---- the V^T fragments of the whole tile are requested NOW (into the registers the K fragments just left): they land
        // while the softmax below keeps the VALU busy, so the PV MFMAs start without an LDS round trip
        h4 v0f[2][2][DT], v1f[2][2][DT];
#pragma unroll
        for (int sub = 0; sub < NSUB; ++sub)
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int t = 0; t < DT; ++t) {
                    const char* vp = Vs + vfrag + t * 32 * VS + (sub * 32 + 16 * s) * 2;
                    v0f[sub][s][t] = *(const h4*)vp;
                    v1f[sub][s][t] = *(const h4*)(vp + 16);
                }
        __builtin_amdgcn_sched_barrier(0);
        if (k0 + 64 > Tk) {   // ragged last tile: keys >= Tk get -inf
#pragma unroll
            for (int sub = 0; sub < NSUB; ++sub)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = k0 + sub * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                    if (key >= Tk) sacc[sub][r] = -INFINITY;
                }
        }
        // ---- online softmax for this lane's query (keys split over the two lane halves), log2 domain
        float psum = 0.f;
        if constexpr (FOLD) {
            // scores arrive as s log2(e) d^-1/2 - m_run; mx is therefore relative to the running max
            float mx = sacc[0][0];
#pragma unroll
            for (int r = 1; r < 16; ++r) mx = fmaxf(mx, sacc[0][r]);
            if constexpr (NSUB == 2) {
#pragma unroll
                for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sacc[1][r]);
            }
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            const bool first = (k0 == 0);
            if (first || !__all(mx <= ATT_THR)) {
                const float m_new = first ? mx : m_run + fmaxf(mx, 0.f);
                const float m_hat = (float)(half_t)m_new;          // the offset must be exactly what Q[q][D] can hold
                const float delta = m_run - m_hat;
                const float alpha = first ? 1.f : __builtin_amdgcn_exp2f(delta);
                m_run = m_hat;
                if constexpr (CAP) cap_l *= alpha;
#pragma unroll
                for (int t = 0; t < DT; ++t)
#pragma unroll
                    for (int r = 0; r < 16; ++r) oacc[t][r] *= alpha;
#pragma unroll
                for (int sub = 0; sub < NSUB; ++sub)
#pragma unroll
                    for (int r = 0; r < 16; ++r) sacc[sub][r] += delta;   // this tile was taken against the old offset
                if (lh == PH) qf[PS][0] = (half_t)(-m_hat);
            }
#pragma unroll
            for (int sub = 0; sub < NSUB; ++sub)
#pragma unroll
                for (int r = 0; r < 16; ++r) sacc[sub][r] = __builtin_amdgcn_exp2f(sacc[sub][r]);
        } else {
        float mx = sacc[0][0];
#pragma unroll
        for (int r = 1; r < 16; ++r) mx = fmaxf(mx, sacc[0][r]);
        if constexpr (NSUB == 2) {
#pragma unroll
            for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sacc[1][r]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32)) * sl2e;
        // raise the running max only when some query of this wave outgrew it by more than ATT_THR (deferred rescale)
        if (!__all(mx - m_run <= ATT_THR)) {
            const float m_new = fmaxf(m_run, mx);
            const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
            m_run = m_new;
            l_run *= alpha;
            if constexpr (CAP) cap_l *= alpha;
#pragma unroll
            for (int t = 0; t < DT; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) oacc[t][r] *= alpha;
        }
#pragma unroll
        for (int sub = 0; sub < NSUB; ++sub)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p = __builtin_amdgcn_exp2f(sacc[sub][r] * sl2e - m_run);
                sacc[sub][r] = p;
                if constexpr (!ONES) psum += p;
            }
        }
        if constexpr (!ONES) l_run += psum;
        if constexpr (CAP) {      // the fp32 probabilities of this tile, against m_run as it stands now (keys >= Tk: no slot, not stored)
#pragma unroll
            for (int j = 0; j < ATT_CAP_MAX_KEYS / 64; ++j)
                cap_m[j] = (j == (k0 >> 6)) ? m_run : cap_m[j];
            float cs = 0.f;
#pragma unroll
            for (int sub = 0; sub < NSUB; ++sub)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    cs += sacc[sub][r];
                    const int key = k0 + sub * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                    if (q < T && key < Tk) cap_row[key] = sacc[sub][r];
                }
            cap_l += cs;
        }

        // ---- O^T += Vt P^T   (with ONES: row D of O^T accumulates sum_k p)
#pragma unroll
        for (int sub = 0; sub < NSUB; ++sub) {
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                h8 pf;
#pragma unroll
                for (int j = 0; j < 8; ++j) pf[j] = (half_t)sacc[sub][8 * s + j];
#pragma unroll
                for (int t = 0; t < DT; ++t) {
                    const h4 v0 = v0f[sub][s][t], v1 = v1f[sub][s][t];
                    const h8 vf = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
                    oacc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf, oacc[t], 0, 0, 0);
                }
            }
        }
        if (more) store_tile(std::integral_constant<int, cur ^ 1>{});     // safe: everyone passed this iteration's barrier after reading cur^1
    };
    using one_t = std::integral_constant<int, 1>;
    using two_t = std::integral_constant<int, 2>;
    for (int k0 = 0; k0 < Tk; k0 += 128) {
        if (k0 + 32 >= Tk) tile(k0, std::integral_constant<int, 0>{}, one_t{});
        else tile(k0, std::integral_constant<int, 0>{}, two_t{});
        if (k0 + 64 < Tk) {
            if (k0 + 96 >= Tk) tile(k0 + 64, std::integral_constant<int, 1>{}, one_t{});
            else tile(k0 + 64, std::integral_constant<int, 1>{}, two_t{});
        }
    }

    if constexpr (CAP) {
        __syncthreads();      // every lane re-reads only what it stored itself; the barrier drains those stores first
        const float cinv = 1.0f / (cap_l + __shfl_xor(cap_l, 32));
#pragma unroll
        for (int j = 0; j < ATT_CAP_MAX_KEYS / 64; ++j)
            if (j * 64 < Tk) {
                const float f = __builtin_amdgcn_exp2f(cap_m[j] - m_run) * cinv;
#pragma unroll
                for (int r = 0; r < 32; ++r) {
                    const int key = j * 64 + (r >> 4) * 32 + (r & 3) + 8 * ((r & 15) >> 2) + 4 * lh;
                    if (q < T && key < Tk) cap_row[key] *= f;
                }
            }
    }
    float l_tot;
    if constexpr (ONES) {
        // row D of O^T lives in tile D/32, register (D%32 -> (r&3)+8(r>>2)+4h): fetch it from the lane half that owns it
        constexpr int rr = D % 32;
        constexpr int reg = (rr & 3) + 4 * (rr >> 3);     // register index within the half that has 4*lh == rr & 4
        constexpr int owner_half = (rr >> 2) & 1;
        const float mine = oacc[D / 32][reg];
        const float other = __shfl_xor(mine, 32);
        l_tot = (lh == owner_half) ? mine : other;
    } else {
        l_tot = l_run + __shfl_xor(l_run, 32);
    }
    const float inv = 1.0f / l_tot;
    if (q < T) {
        half_t* op = O + ((size_t)b * T + q) * ldo + head * D;
#pragma unroll
        for (int t = 0; t < DT; ++t)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int dd = t * 32 + 8 * g + 4 * lh;
                if (dd < D) {
                    h4 pk = {(half_t)(oacc[t][4 * g] * inv), (half_t)(oacc[t][4 * g + 1] * inv),
                             (half_t)(oacc[t][4 * g + 2] * inv), (half_t)(oacc[t][4 * g + 3] * inv)};
                    *(h4*)(op + dd) = pk;
                }
            }
    }
}

// =====================================================================================================================
// Text cross-attention, key-resident (64 < Tk <= 256: one, two or three 77-token parts joined along the token axis, cldm.py:836-849 /
// hack.py:23-68).  The kernel above gives every 128 queries their own workgroup, which stages K / V^T tile by tile behind barriers:
// with two tiles of keys that is three dependent memory round trips and two barriers for 50 MFMAs -- latency-bound at 2.2 TB/s of
// Q + O traffic (72 us at T = 4096, d = 40).  Here a workgroup stages ALL keys of its (batch, head) once (K [32 NS][DP], V^T [d][32 NS]
// with the ones row), passes ONE barrier, and then each of its four waves walks cpw chunks of 32 queries on its own: S^T = K Q^T for
// the NS 32-key sub-tiles in one go, a plain (single-pass) softmax -- the maximum over all NS score tiles before any exp2: a spike
// may sit in any of them -- and O^T = V^T P^T; the next chunk's Q rows are requested before the current chunk is computed.  Heads run
// fastest over workgroups (see above).
// CONTRACT: NS == ceil(Tk / 32), so that only sub-tile NS - 1 can hold keys >= Tk and needs the mask (launch_cross returns
// FGDM_ERR_ARG for anything else).
// LDS: NS = 3 (the 77 text tokens) fits the static 64 KB; K / V^T for 256 keys need up to 123 KB (d = 80), so NS >= 4 is dynamic;
// d = 160 fits up to NS = 7 (155 KB) and falls back to attn_kernel beyond.  At NS = 8 the scores alone are 128 fp32 registers per
// lane: the kernel runs at one workgroup per CU by LDS anyway, so the 512-register budget of one wave per SIMD is its to use.
constexpr int attn_cross_lds(int D, int NS) {
    const int DP = (D + 15) / 16 * 16, DT = (D + 31) / 32, KEYS = NS * 32;
    return KEYS * (DP * 2 + 16) + DT * 32 * (KEYS * 2 + 72) + (D <= 80 ? 4 * 32 * (D * 2 + 8) : 0);
}
template <int D, int NS, class... Cap>
__global__ __launch_bounds__(256) void attn_cross_kernel(const half_t* __restrict__ Q, int ldq,
                                                         const half_t* __restrict__ K, int ldk,
                                                         const half_t* __restrict__ Vt, int ldvt,
                                                         half_t* __restrict__ O, int ldo,
                                                         int H, int T, int Tk, float sl2e, int cpw, Cap... cap) {
    constexpr bool CAP = sizeof...(Cap) > 0;      // the capturing instantiation (see att_cap_plane above)
    constexpr int KEYS = NS * 32;
    constexpr int DP = (D + 15) / 16 * 16, NKS = DP / 16, DT = (D + 31) / 32;
    constexpr bool ONES = (DT * 32 > D);
    constexpr bool FOLD = (DP > D) && (D % 8 == 0);      // same Q scaling rule as attn_kernel (the spare slot itself stays 0 here)
    constexpr int KS = DP * 2 + 16;            // K row stride (bytes): odd multiple of 16
    constexpr int VS = KEYS * 2 + 72;          // V^T row stride: 66 dwords = 2 mod 32 -> b64 reads conflict-free like the 34 above
    constexpr int DC = D / 8;
    // Q rows enter and O rows leave through a wave-private [32][D] LDS tile, so that global memory sees 16-byte pieces of whole
    // 2 D-byte row slices (a lane per query row means 64 different lines per instruction, 8 bytes each on the way out)
    constexpr bool RELAY = D <= 80;
    constexpr int RS = D * 2 + 8;              // 22 / 42 dwords per row: 8-byte accesses of 16 consecutive rows hit 16 banks
    constexpr int PCS = 32 * (D / 8), KP = (PCS + 63) / 64;      // 16-byte pieces of a 32-row chunk; per lane
    static_assert(attn_cross_lds(D, NS) == KEYS * KS + DT * 32 * VS + (RELAY ? 4 * 32 * RS : 0), "LDS size formula");
    char* smem;
    if constexpr (NS == 3) {                   // static: its addresses are immediates (a dynamic base costs ~4 % more instructions)
        __shared__ __attribute__((aligned(16))) char smem_static[attn_cross_lds(D, NS)];
        smem = smem_static;
    } else {                                   // beyond the static 64 KB
        extern __shared__ __attribute__((aligned(16))) char smem_dynamic[];
        smem = smem_dynamic;
    }
    char* Ks = smem;
    char* Vs = smem + KEYS * KS;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lq = lane & 31, lh = lane >> 5;
    const int qpw = 128 * cpw;                               // queries per workgroup
    const int ncb = (T + qpw - 1) / qpw;
    const int logical = att_logical_block();
    const int head = logical % H, rest = logical / H;
    const int cblk = rest % ncb, b = rest / ncb;

    const half_t* Kb = K + (size_t)b * Tk * ldk + head * D;
    const half_t* Vb = Vt + ((size_t)b * H + head) * D * ldvt;
    // ---- stage K (rows past Tk repeat the last valid one: their scores are masked) and V^T (rows are padded to 64-key multiples):
    // every global load of the workgroup is issued before the first LDS store -- ONE memory round trip (as loops of load / store
    // pairs the staging was 5-6 dependent round trips, most of a workgroup's life)
    constexpr int KPC = KEYS * (DP / 8), VPC = DT * 32 * (KEYS / 8);
    constexpr int KPT = (KPC + 255) / 256, VPT = (VPC + 255) / 256;
    h8 kst[KPT], vst[VPT];
#pragma unroll
    for (int u = 0; u < KPT; ++u) {
        const int i = tid + 256 * u, key = i / (DP / 8), c = i - key * (DP / 8);
        kst[u] = (h8)(half_t)0;
        if (i < KPC && c < DC) kst[u] = *(const h8*)(Kb + (size_t)min(key, Tk - 1) * ldk + c * 8);
    }
#pragma unroll
    for (int u = 0; u < VPT; ++u) {
        const int i = tid + 256 * u, r = i / (KEYS / 8), c = i - r * (KEYS / 8);
        vst[u] = (r == D) ? (h8)(half_t)1 : (h8)(half_t)0;
        if (i < VPC && r < D) vst[u] = *(const h8*)(Vb + (size_t)r * ldvt + c * 8);
    }
    char* scr = smem + KEYS * KS + DT * 32 * VS + (threadIdx.x >> 6) * 32 * RS;      // this wave's tile
    // the chunk's Q rows: per-lane fragments straight from global memory, or (RELAY) 16-byte pieces in row order
    constexpr int NQ = RELAY ? KP : NKS;
    auto load_q = [&](int q0, h8 (&qr)[NQ]) {      // q0: first query of the chunk (wave-uniform)
        if constexpr (RELAY) {
#pragma unroll
            for (int u = 0; u < KP; ++u) {
                const int c = lane + 64 * u, row = c / (D / 8), ck = c - row * (D / 8);
                qr[u] = (h8)(half_t)0;
                if (c < PCS && q0 + row < T) qr[u] = *(const h8*)(Q + ((size_t)b * T + q0 + row) * ldq + head * D + ck * 8);
            }
        } else {
#pragma unroll
            for (int s2 = 0; s2 < NKS; ++s2) {
                const int c = 16 * s2 + 8 * lh;
                qr[s2] = (h8)(half_t)0;
                if (c < D && q0 + lq < T) qr[s2] = *(const h8*)(Q + ((size_t)b * T + q0 + lq) * ldq + head * D + c);
            }
        }
    };
    const int q_first = cblk * qpw + wave * 32;              // chunk i of this wave: queries q_first + i * 128 + [0, 32)
    h8 qn[NQ];
    load_q(q_first, qn);
#pragma unroll
    for (int u = 0; u < KPT; ++u) {
        const int i = tid + 256 * u, key = i / (DP / 8), c = i - key * (DP / 8);
        if (i < KPC) *(h8*)(Ks + key * KS + c * 16) = kst[u];
    }
#pragma unroll
    for (int u = 0; u < VPT; ++u) {
        const int i = tid + 256 * u, r = i / (KEYS / 8), c = i - r * (KEYS / 8);
        if (i < VPC) {
            const h8 v = vst[u];
            const h4 lo = {v[0], v[1], v[2], v[3]}, hi = {v[4], v[5], v[6], v[7]};
            *(h4*)(Vs + r * VS + c * 16) = lo;
            *(h4*)(Vs + r * VS + c * 16 + 8) = hi;
        }
    }
    __syncthreads();

    const int kfrag = lq * KS + 8 * lh * 2, vfrag = lq * VS + 4 * lh * 2;
    for (int i = 0; i < cpw; ++i) {
        const int q0 = __builtin_amdgcn_readfirstlane(q_first + i * 128);
        if (q0 >= T) break;                                  // wave-uniform: this chunk starts past the end
        const int q = q0 + lq;
        h8 qf[NKS];
        if constexpr (RELAY) {
#pragma unroll
            for (int u = 0; u < KP; ++u) {
                const int c = lane + 64 * u, row = c / (D / 8), ck = c - row * (D / 8);
                if (c < PCS) {
                    const h4 lo = {qn[u][0], qn[u][1], qn[u][2], qn[u][3]}, hi = {qn[u][4], qn[u][5], qn[u][6], qn[u][7]};
                    *(h4*)(scr + row * RS + ck * 16) = lo;
                    *(h4*)(scr + row * RS + ck * 16 + 8) = hi;
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
            for (int s2 = 0; s2 < NKS; ++s2) {
                const int c = 16 * s2 + 8 * lh;
                qf[s2] = (h8)(half_t)0;
                if (c < D) {
                    const h4 lo = *(const h4*)(scr + lq * RS + c * 2), hi = *(const h4*)(scr + lq * RS + c * 2 + 8);
                    qf[s2] = h8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // fragments read before the tile is reused for O
        } else {
#pragma unroll
            for (int s2 = 0; s2 < NKS; ++s2) qf[s2] = qn[s2];
        }
        if (i + 1 < cpw) load_q(q0 + 128, qn);
        if constexpr (FOLD) {
#pragma unroll
            for (int s2 = 0; s2 < NKS; ++s2)
#pragma unroll
                for (int j = 0; j < 8; ++j) qf[s2][j] = (half_t)((float)qf[s2][j] * sl2e);
        }
        // ---- S^T = K Q^T, all keys
        f32x16 sacc[NS];
#pragma unroll
        for (int sub = 0; sub < NS; ++sub) {
#pragma unroll
            for (int r = 0; r < 16; ++r) sacc[sub][r] = 0.f;
#pragma unroll
            for (int s2 = 0; s2 < NKS; ++s2) {
                const h8 kf = *(const h8*)(Ks + kfrag + sub * 32 * KS + 16 * s2 * 2);
                sacc[sub] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[s2], sacc[sub], 0, 0, 0);
            }
        }
        // Only the last sub-tile can hold keys >= Tk (the contract: NS == ceil(Tk / 32)), and it is masked without a test.  Three
        // instantiations ran 0.3 - 3 % slower in that form than with every sub-tile from 1 on masked behind a wave-uniform test (the
        // compiler schedules the chunk differently; profiles/attention_text_kernel_unified.txt): they keep the form with the test
        constexpr int MASK_FROM = ((D == 160 && (NS == 5 || NS == 6)) || (D == 80 && NS == 8)) ? 1 : NS - 1;
#pragma unroll
        for (int sub = MASK_FROM; sub < NS; ++sub)
            if (MASK_FROM == NS - 1 || (sub + 1) * 32 > Tk) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = sub * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                    if (key >= Tk) sacc[sub][r] = -INFINITY;
                }
            }
        float mx = sacc[0][0];
#pragma unroll
        for (int sub = 0; sub < NS; ++sub)
#pragma unroll
            for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sacc[sub][r]);
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float sc = FOLD ? 1.0f : sl2e;
        float psum = 0.f;
#pragma unroll
        for (int sub = 0; sub < NS; ++sub)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float pv = __builtin_amdgcn_exp2f((sacc[sub][r] - mx) * sc);
                sacc[sub][r] = pv;
                if constexpr (!ONES) psum += pv;
            }
        if constexpr (CAP) {      // all keys are here: the row's maximum and its fp32 sum are final before V^T P^T
            float cs = 0.f;
#pragma unroll
            for (int sub = 0; sub < NS; ++sub)
#pragma unroll
                for (int r = 0; r < 16; ++r) cs += sacc[sub][r];      // masked keys: exp2(-inf) = 0
            const float cinv = 1.0f / (cs + __shfl_xor(cs, 32));
            if (q < T) {
                float* cap_row = att_cap_plane(cap...) + (((size_t)b * H + head) * T + q) * Tk;
#pragma unroll
                for (int sub = 0; sub < NS; ++sub)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int key = sub * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                        if (key < Tk) cap_row[key] = sacc[sub][r] * cinv;
                    }
            }
        }
        // ---- O^T = V^T P^T (row D of O^T: the sum of the fp16 probabilities)
        f32x16 oacc[DT];
#pragma unroll
        for (int t = 0; t < DT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) oacc[t][r] = 0.f;
#pragma unroll
        for (int sub = 0; sub < NS; ++sub)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                h8 pf;
#pragma unroll
                for (int j = 0; j < 8; ++j) pf[j] = (half_t)sacc[sub][8 * s2 + j];
#pragma unroll
                for (int t = 0; t < DT; ++t) {
                    const char* vp = Vs + vfrag + t * 32 * VS + (sub * 32 + 16 * s2) * 2;
                    const h4 v0 = *(const h4*)vp, v1 = *(const h4*)(vp + 16);
                    const h8 vf = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
                    oacc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf, oacc[t], 0, 0, 0);
                }
            }
        float l_tot;
        if constexpr (ONES) {
            constexpr int rr = D % 32;
            constexpr int reg = (rr & 3) + 4 * (rr >> 3);
            constexpr int owner_half = (rr >> 2) & 1;
            const float mine = oacc[D / 32][reg];
            const float other = __shfl_xor(mine, 32);
            l_tot = (lh == owner_half) ? mine : other;
        } else {
            l_tot = psum + __shfl_xor(psum, 32);
        }
        const float inv = 1.0f / l_tot;
        if constexpr (RELAY) {
#pragma unroll
            for (int t = 0; t < DT; ++t)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int dd = t * 32 + 8 * g + 4 * lh;
                    if (dd < D) {
                        h4 pk = {(half_t)(oacc[t][4 * g] * inv), (half_t)(oacc[t][4 * g + 1] * inv),
                                 (half_t)(oacc[t][4 * g + 2] * inv), (half_t)(oacc[t][4 * g + 3] * inv)};
                        *(h4*)(scr + lq * RS + dd * 2) = pk;
                    }
                }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
            for (int u = 0; u < KP; ++u) {
                const int c = lane + 64 * u, row = c / (D / 8), ck = c - row * (D / 8);
                if (c < PCS && q0 + row < T) {
                    const h4 lo = *(const h4*)(scr + row * RS + ck * 16), hi = *(const h4*)(scr + row * RS + ck * 16 + 8);
                    *(h8*)(O + ((size_t)b * T + q0 + row) * ldo + head * D + ck * 8) = h8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // the tile is free for the next chunk's Q
        } else if (q < T) {
            half_t* op = O + ((size_t)b * T + q) * ldo + head * D;
#pragma unroll
            for (int t = 0; t < DT; ++t)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int dd = t * 32 + 8 * g + 4 * lh;
                    if (dd < D) {
                        h4 pk = {(half_t)(oacc[t][4 * g] * inv), (half_t)(oacc[t][4 * g + 1] * inv),
                                 (half_t)(oacc[t][4 * g + 2] * inv), (half_t)(oacc[t][4 * g + 3] * inv)};
                        *(h4*)(op + dd) = pk;
                    }
                }
        }
    }
}


// =====================================================================================================================
// Ping-pong variant for long self-attention (round 2).  PMC on the kernel above (T = Tk = 4096, d = 40): per SIMD the matrix
// pipe is busy 40 % of the time and the vector ALU 52 % -- and the two hardly ever at the same moment: three free-running
// waves per SIMD drift into the same phase, all in their softmax, then all in their MFMAs.  Here a workgroup has EIGHT waves,
// two per SIMD: group A (waves 0-3) and group B (waves 4-7) own 128 queries each and run the SAME program one barrier apart,
// so that on every SIMD one wave is in its MFMA slot {P V of tile k, Q K^T of tile k+1} while its partner is in its VALU slot
// {softmax of tile k, LDS writes of the next K / V^T tile}; two raw s_barriers per tile keep them there.
//   slot:      0        1        2        3        4   ...
//   group A:  QK(0)    X(0)     Y(0)     X(1)     Y(1)          X(k) = softmax(k) + stage tile, Y(k) = PV(k) + QK(k+1)
//   group B:   -       QK(0)    X(0)     Y(0)     X(1)
// K / V^T live in LDS as PAIRS p(j) = (K tile j+1, V^T tile j), double-buffered (buffer j & 1; K tile 0 is "p(-1)"): p(j) is
// read in slots 2j+2 (A) and 2j+3 (B), each wave writes its share of it in its own X phase -- A in X(j) (slot 2j+1), B in
// X(j-1) (slot 2j) -- which is after the last read of p(j-2) (slot 2j-1) and before the first read of p(j).  Every wave
// executes the same number of barriers (B one extra at the start, A one extra at the end).
// (measured and rejected around this kernel, and the software-pipelined variants of rounds 2 and 3: DESIGN.md section 4.2 / 4.3)
template <int D>
__global__ __launch_bounds__(512) void attn_pp_kernel(const half_t* __restrict__ Q, int ldq,
                                                      const half_t* __restrict__ K, int ldk,
                                                      const half_t* __restrict__ Vt, int ldvt,
                                                      half_t* __restrict__ O, int ldo,
                                                      int H, int T, int Tk, float sl2e) {
    constexpr int DP = (D + 15) / 16 * 16, NKS = DP / 16, DT = (D + 31) / 32;
    constexpr bool ONES = (DT * 32 > D);
    constexpr bool FOLD = (DP > D) && (D % 8 == 0);
    constexpr int PS = D / 16, PH = (D % 16) / 8;
    constexpr int KS = DP * 2 + 16, VS = 64 * 2 + 8, DC = D / 8;
    constexpr int NCH = 64 * DC;                    // 16-byte chunks of a K tile = of a V^T tile (D * 8)
    constexpr int CH = (NCH + 511) / 512;           // chunks per thread per tile
    constexpr int KBYTES = 64 * KS, VBYTES = DT * 32 * VS, PAIR = KBYTES + VBYTES;
    __shared__ __attribute__((aligned(16))) char smem[2 * PAIR];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = wave >> 2;                      // 0 = A, 1 = B
    const int lq = lane & 31, lh = lane >> 5;
    const int nqb = (T + 255) / 256;
    const int logical = att_logical_block();
    const int qblk = logical % nqb, bh = logical / nqb;
    const int b = bh / H, head = bh - b * H;
    const int q = qblk * 256 + wave * 32 + lq;
    const int nt = (Tk + 63) / 64;

    // pad regions of both buffers, written once (visible after the prologue barrier)
    for (int buf = 0; buf < 2; ++buf) {
        char* Ksb = smem + buf * PAIR;
        char* Vsb = Ksb + KBYTES;
        if constexpr (DP > D) {
            for (int i = tid; i < 64 * (DP - D) / 8; i += 512) {
                const int key = i / ((DP - D) / 8), c = i % ((DP - D) / 8);
                h8 pad = (h8)(half_t)0;
                if (FOLD && c == 0) pad[0] = (half_t)1;
                *(h8*)(Ksb + key * KS + (D + c * 8) * 2) = pad;
            }
        }
        for (int i = tid; i < (DT * 32 - D) * 16; i += 512) {
            const int r = D + i / 16, c = i % 16;
            *(h4*)(Vsb + r * VS + c * 8) = (r == D) ? (h4)(half_t)1 : (h4)(half_t)0;
        }
    }

    h8 qf[NKS];
#pragma unroll
    for (int s = 0; s < NKS; ++s) {
        const int c = 16 * s + 8 * lh;
        qf[s] = (h8)(half_t)0;
        if (c < D && q < T) qf[s] = *(const h8*)(Q + ((size_t)b * T + q) * ldq + head * D + c);
        if constexpr (FOLD) {
#pragma unroll
            for (int j = 0; j < 8; ++j) qf[s][j] = (half_t)((float)qf[s][j] * sl2e);
        }
    }
    f32x16 oacc[DT];
#pragma unroll
    for (int t = 0; t < DT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[t][r] = 0.f;
    float m_run = FOLD ? 0.f : -INFINITY, l_run = 0.f;

    const half_t* Kb = K + (size_t)b * Tk * ldk + head * D;
    const half_t* Vb = Vt + ((size_t)b * H + head) * D * ldvt;

    // per-thread, loop-invariant parts of the tile copy; chunk validity is wave-uniform (NCH is a multiple of 64)
    int k_goff[CH], k_loff[CH], k_key[CH], v_goff[CH], v_loff[CH];
#pragma unroll
    for (int u = 0; u < CH; ++u) {
        const int i = tid + u * 512;
        const int key = i / DC, c = i - key * DC;
        k_key[u] = key; k_goff[u] = key * ldk + c * 8; k_loff[u] = key * KS + c * 16;
        const int r = i >> 3, cv = i & 7;
        v_goff[u] = r * ldvt + cv * 8; v_loff[u] = r * VS + cv * 16;
    }
    h8 kreg[CH], vreg[CH];
    // K tile kt and V^T tile vtile -> registers (either may be absent: kt >= nt / vtile < 0)
    auto load_pair = [&](int kt, int vtile) {
        if (kt < nt) {
            const int k0 = kt * 64;
            const half_t* kb = Kb + (size_t)k0 * ldk;
            const bool ragged = k0 + 64 > Tk;
#pragma unroll
            for (int u = 0; u < CH; ++u)
                if ((u * 8 + wave) * 64 < NCH) {
                    int off = k_goff[u];
                    if (ragged) off += (min(k_key[u], Tk - 1 - k0) - k_key[u]) * ldk;
                    kreg[u] = *(const h8*)(kb + off);
                }
        }
        if (vtile >= 0 && vtile < nt) {
            const half_t* vb = Vb + vtile * 64;
#pragma unroll
            for (int u = 0; u < CH; ++u)
                if ((u * 8 + wave) * 64 < NCH) vreg[u] = *(const h8*)(vb + v_goff[u]);
        }
    };
    auto store_pair = [&](int kt, int vtile, int buf) {
        char* Ksb = smem + buf * PAIR;
        char* Vsb = Ksb + KBYTES;
        if (kt < nt) {
#pragma unroll
            for (int u = 0; u < CH; ++u)
                if ((u * 8 + wave) * 64 < NCH) *(h8*)(Ksb + k_loff[u]) = kreg[u];
        }
        if (vtile >= 0 && vtile < nt) {
#pragma unroll
            for (int u = 0; u < CH; ++u)
                if ((u * 8 + wave) * 64 < NCH) {
                    const h8 v = vreg[u];
                    h4 lo = {v[0], v[1], v[2], v[3]}, hi = {v[4], v[5], v[6], v[7]};
                    *(h4*)(Vsb + v_loff[u]) = lo;
                    *(h4*)(Vsb + v_loff[u] + 8) = hi;
                }
        }
    };
    auto barrier = [&]() { __syncthreads(); };    // workgroup-scope fences + s_barrier: LDS traffic drained, global prefetches stay in flight
    const int kfrag = lq * KS + 8 * lh * 2, vfrag = lq * VS + 4 * lh * 2;

    f32x16 sacc[2];
    h8 pf[2][2];                       // fp16 probabilities of the tile: the B operand of P V
    auto qk = [&](int buf) {           // S^T = K Q^T of the K tile in `buf`
        const char* Ks = smem + buf * PAIR;
        h8 kf[2][NKS];
#pragma unroll
        for (int sub = 0; sub < 2; ++sub)
#pragma unroll
            for (int s = 0; s < NKS; ++s) kf[sub][s] = *(const h8*)(Ks + kfrag + sub * 32 * KS + 16 * s * 2);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
#pragma unroll
            for (int r = 0; r < 16; ++r) sacc[sub][r] = 0.f;
#pragma unroll
            for (int s = 0; s < NKS; ++s) sacc[sub] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[sub][s], qf[s], sacc[sub], 0, 0, 0);
        }
    };
    auto pv = [&](int buf) {           // O^T += V^T P^T with the V^T tile in `buf`
        const char* Vs = smem + buf * PAIR + KBYTES;
#pragma unroll
        for (int sub = 0; sub < 2; ++sub)
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int t = 0; t < DT; ++t) {
                    const char* vp = Vs + vfrag + t * 32 * VS + (sub * 32 + 16 * s) * 2;
                    const h4 v0 = *(const h4*)vp, v1 = *(const h4*)(vp + 16);
                    const h8 vf = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
                    oacc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf[sub][s], oacc[t], 0, 0, 0);
                }
    };
    auto softmax = [&](int k0, bool first) {      // sacc -> pf (online softmax in the log2 domain, deferred rescale)
        if (k0 + 64 > Tk) {
#pragma unroll
            for (int sub = 0; sub < 2; ++sub)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = k0 + sub * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                    if (key >= Tk) sacc[sub][r] = -INFINITY;
                }
        }
        float psum = 0.f;
        if constexpr (FOLD) {
            float mx = fmaxf(sacc[0][0], sacc[1][0]);
#pragma unroll
            for (int r = 1; r < 16; ++r) mx = fmaxf(fmaxf(mx, sacc[0][r]), sacc[1][r]);
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            if (first || !__all(mx <= ATT_THR)) {
                const float m_new = first ? mx : m_run + fmaxf(mx, 0.f);
                const float m_hat = (float)(half_t)m_new;
                const float delta = m_run - m_hat;
                const float alpha = first ? 1.f : __builtin_amdgcn_exp2f(delta);
                m_run = m_hat;
#pragma unroll
                for (int t = 0; t < DT; ++t)
#pragma unroll
                    for (int r = 0; r < 16; ++r) oacc[t][r] *= alpha;
#pragma unroll
                for (int sub = 0; sub < 2; ++sub)
#pragma unroll
                    for (int r = 0; r < 16; ++r) sacc[sub][r] += delta;
                if (lh == PH) qf[PS][0] = (half_t)(-m_hat);
            }
#pragma unroll
            for (int sub = 0; sub < 2; ++sub)
#pragma unroll
                for (int r = 0; r < 16; ++r) sacc[sub][r] = __builtin_amdgcn_exp2f(sacc[sub][r]);
        } else {
            float mx = fmaxf(sacc[0][0], sacc[1][0]);
#pragma unroll
            for (int r = 1; r < 16; ++r) mx = fmaxf(mx, fmaxf(sacc[0][r], sacc[1][r]));
            mx = fmaxf(mx, __shfl_xor(mx, 32)) * sl2e;
            if (!__all(mx - m_run <= ATT_THR)) {
                const float m_new = fmaxf(m_run, mx);
                const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
                m_run = m_new;
                l_run *= alpha;
#pragma unroll
                for (int t = 0; t < DT; ++t)
#pragma unroll
                    for (int r = 0; r < 16; ++r) oacc[t][r] *= alpha;
            }
#pragma unroll
            for (int sub = 0; sub < 2; ++sub)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float p = __builtin_amdgcn_exp2f(sacc[sub][r] * sl2e - m_run);
                    sacc[sub][r] = p;
                    if constexpr (!ONES) psum += p;
                }
        }
        if constexpr (!ONES) l_run += psum;
#pragma unroll
        for (int sub = 0; sub < 2; ++sub)
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int j = 0; j < 8; ++j) pf[sub][s][j] = (half_t)sacc[sub][8 * s + j];
    };

    // ---- prologue: K tile 0 ("pair -1") into buffer 1; group B also writes its shares of pair 0 = (K tile 1, V^T tile 0)
    load_pair(0, -1);
    store_pair(0, -1, 1);
    if (grp == 1) {
        load_pair(1, 0);
        store_pair(1, 0, 0);
    }
    load_pair(1 + grp, grp);           // the pair this wave writes in X(0): A pair 0, B pair 1
    barrier();
    if (grp == 1) barrier();           // group B runs one slot behind group A
    qk(1);                             // Q K^T of tile 0
    for (int k = 0; k < nt; ++k) {
        barrier();
        // ---- X(k): VALU slot
        softmax(k * 64, k == 0);
        {
            const int j = k + grp;                         // pair written in this phase (pair j = K tile j+1, V^T tile j)
            if (j < nt) store_pair(j + 1, j, j & 1);
            if (j + 1 < nt) load_pair(j + 2, j + 1);       // ... and the one after it starts its trip from HBM / L2
        }
        barrier();
        // ---- Y(k): matrix slot
        pv(k & 1);
        if (k + 1 < nt) qk(k & 1);                         // K tile k+1 travels in pair k
    }
    if (grp == 0) barrier();

    float l_tot;
    if constexpr (ONES) {
        constexpr int rr = D % 32;
        constexpr int reg = (rr & 3) + 4 * (rr >> 3);
        constexpr int owner_half = (rr >> 2) & 1;
        const float mine = oacc[D / 32][reg];
        const float other = __shfl_xor(mine, 32);
        l_tot = (lh == owner_half) ? mine : other;
    } else {
        l_tot = l_run + __shfl_xor(l_run, 32);
    }
    const float inv = 1.0f / l_tot;
    if (q < T) {
        half_t* op = O + ((size_t)b * T + q) * ldo + head * D;
#pragma unroll
        for (int t = 0; t < DT; ++t)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int dd = t * 32 + 8 * g + 4 * lh;
                if (dd < D) {
                    h4 pk = {(half_t)(oacc[t][4 * g] * inv), (half_t)(oacc[t][4 * g + 1] * inv),
                             (half_t)(oacc[t][4 * g + 2] * inv), (half_t)(oacc[t][4 * g + 3] * inv)};
                    *(h4*)(op + dd) = pk;
                }
            }
    }
}

// =====================================================================================================================
// Two-strand kernel for long self-attention (round 4).  What bounds the kernels above at d = 40 is the SUM of a wave's matrix and
// vector-ALU time (vector instructions of ANOTHER wave hardly enter a wave's MFMA shadows; instructions of the
// SAME wave do), and 1.4x the algorithmic MFMAs.  Here one wave owns 64 queries as two independent 32-query STRANDS A and B, and its
// instruction stream is written so that every MFMA of one strand is followed by softmax work of the other:
//   * S^T = K Q^T runs on v_mfma_f32_32x32x16_f16 (keys on the rows; the contraction carries one slot more than d, d = 40 -> 48,
//     for the scale / running-max fold: K[:, d] = 1, Q[:, d] = -max);
//   * K / V^T tiles arrive by LDS-DMA (global_load_lds_dwordx4) into a ring of three 64-key slots, two tiles ahead, one raw
//     s_barrier per tile: no staging registers, no ds_write, no second barrier.  Both images are ROW-major like their sources (a
//     wave instruction fetches whole rows), conflict-free for the fragment reads: V^T rows of 128 bytes with their 16-byte pieces
//     XOR-swizzled on the SOURCE side by (row >> 1) & 7, K rows of 16 d / 8 bytes (see KXOR / ROT in the kernel); the K pieces of the
//     fold slot ([1 0 0 0 0 0 0 0], zeros) live in constant LDS pieces behind the ring that the pad lanes read instead;
//   * the K rows of a tile sit in LDS in the order that makes the eight keys of a lane's slice of the B operand P^T CONTIGUOUS in
//     V^T, so a V^T fragment is one ds_read_b128;
//   * four waves per workgroup (ATT_TS_Q = 256 queries), two workgroups per CU at d = 40: the two waves of a SIMD belong to
//     different workgroups and drift apart instead of meeting at the same barrier (eight waves, one workgroup of 512 queries per
//     CU, would halve the L2 -> LDS bytes and lose that).
// Needs T % ATT_TS_Q == 0 and Tk % 64 == 0 (the self-attention shapes).
//
// O^T += V^T P^T comes in two forms, the policy types Pv16 / Pv32 below; everything else stands once, in attn_two_strand_kernel.
//   Pv16  v_mfma_f32_16x16x32_f16: three 16-row tiles cover d = 40 (+ the ones row) instead of two 32-row tiles, 192 instead of 256
//         matrix cycles per 32 x 64 block.  The fp16 probabilities reach the B-operand layout of the 16-wide shape by FOUR
//         v_permlane16_swap per 32 keys: lane n keeps the key groups of query n, lane n + 16 hands over its own in exchange.  The
//         ones row of V^T and its zero padding are constant LDS pieces as well.  Reached under FGDM_ATTN_DQ=1 (d = 40 only).
//   Pv32  v_mfma_f32_32x32x16_f16 again (after the ablations of the 16-wide form: the kernel's time is the SUM of its vector-ALU
//         issue cycles and 8 issue cycles per MFMA -- the matrix pipe's own time hides in the shadows -- so what counts is the
//         NUMBER of MFMAs and of vector instructions, not the matrix cycles): 8 MFMAs per 32 x 64 block instead of 12, no permlane
//         swaps (the S^T accumulators, converted, ARE the B operand), O^T as two 32-row tiles (d = 40 -> 64, rows 41.. zero).  The
//         constant rows of V^T (ones row, zero rows) are part of the LDS image (written once per slot; the DMA fills rows
//         0 .. D - 1 only).  The default at d = 40, 64 and 80; d > 40 runs at one wave per SIMD (two strands need ~280 registers).
__device__ __forceinline__ void att_dma16(unsigned voff, const void* sbase, unsigned lds_wave_addr) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(sbase), "s"(lds_wave_addr) : "memory", "m0");
}
template <int N> __device__ __forceinline__ void att_wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
constexpr int ATT_TS_Q = 256;      // queries per workgroup = its threads: four waves of 64 queries (two 32-query strands) each

// A V^T P^T form carries: DT (O^T tiles), VBYTES (V^T bytes per slot), MIN_BLOCKS (workgroups per CU for __launch_bounds__), C_ZERO
// (offset of the zero piece among the constants), key_of_row (the K row order inside a 32-key sub-tile), init_lds (the constant parts
// of the LDS image), its fragments (V^T, packed probabilities, O^T) with rd_v / pack / mma / rescale / store, and the schedule facts
// of a tile: the NRD V^T fragment reads in the order they are issued, the first RD_B of them between the MFMAs of stage (b) and the
// rest from the second sub-tile of stage (c) on, and the V^T P^T steps of stage (d) (NPV per 32-key sub-tile and strand) at which
// strand B's two max_part calls and its att_max_cross run.
template <int D>
struct Pv16 {
    static constexpr int DT = (D + 16) / 16;                 // 16-row tiles of O^T; row D carries the softmax denominator
    static constexpr int VBYTES = D * 128, MIN_BLOCKS = 2, C_ZERO = 32;
    static constexpr int NPV = DT * 2, NRD = DT * 2, RD_B = NRD;
    static constexpr int MAXB0 = 1, MAXB1 = 3, MAXBX = 4;
    static_assert(((D / 8 * 16) / 4) % 8 == 4, "K rows unswizzled (nothing instantiates the 16-wide form beyond d = 40)");
    // LDS row rho = 8 a + 4 b + c holds key 16 b + 4 a + c, so that the keys whose probabilities end up in lane group g of the
    // 16-wide B operand (after the permlane16 swaps) are keys 8 g .. 8 g + 7
    static __device__ __forceinline__ int key_of_row(int rho) { return 16 * ((rho >> 2) & 1) + 4 * (rho >> 3) + (rho & 3); }
    // constant pieces: [1 0 0 0 0 0 0 0] (K[:, D] of the fold), eight ones (row D of V^T), zeros
    static __device__ __forceinline__ void init_lds(char* smem, char* cst, int slots, int slot_bytes, int kbytes, int tid) {
        if (tid < 3) {
            h8 v = (h8)(half_t)0;
            if (tid == 0) v[0] = (half_t)1;
            if (tid == 1) v = (h8)(half_t)1;
            *(h8*)(cst + tid * 16) = v;
        }
    }

    int n16, g;                                              // O^T layout: query on lane & 15, row quad on lane >> 4
    int v_lane[2];                                           // V^T: row 16 t + n16, source piece 4 sub + g at position (4 sub + g) ^ ((n16 >> 1) & 7)
    const char* c_ones, *c_zero;
    h8 vf[DT][2], pb[2][2][2];
    f32x4 oacc[2][DT][2];
    __device__ __forceinline__ Pv16(int lane, int kbytes, const char* cst) : n16(lane & 15), g(lane >> 4), c_ones(cst + 16), c_zero(cst + C_ZERO) {
#pragma unroll
        for (int X = 0; X < 2; ++X)
#pragma unroll
            for (int t = 0; t < DT; ++t)
#pragma unroll
                for (int qg = 0; qg < 2; ++qg) oacc[X][t][qg] = f32x4{0.f, 0.f, 0.f, 0.f};
        v_lane[0] = kbytes + n16 * 128 + ((g ^ ((n16 >> 1) & 7)) * 16);
        v_lane[1] = kbytes + n16 * 128 + (((4 + g) ^ ((n16 >> 1) & 7)) * 16);
    }
    __device__ __forceinline__ void rd_v(const char* sl, int n) {
        const int t = n % DT, sub = n / DT;
        const char* p = sl + v_lane[sub] + t * 16 * 128;
        if (16 * t + 15 >= D) {                              // rows >= D of the last tile: the ones row, then zeros
            const int d = 16 * t + n16;
            p = d < D ? p : (d == D ? c_ones : c_zero);
        }
        vf[t][sub] = *(const h8*)p;
    }
    // fp16 probabilities of one 32-key sub-tile -> the two B operands (queries 0-15 / 16-31 of the strand) of the 16-wide MFMA
    __device__ __forceinline__ void pack(int X, int sub, const f32x16& s) {
        unsigned pk[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const h2 t2 = {(half_t)s[2 * i], (half_t)s[2 * i + 1]};
            pk[i] = __builtin_bit_cast(unsigned, t2);
        }
        u32x4 lo, hi;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const auto r2 = __builtin_amdgcn_permlane16_swap(pk[i], pk[i + 4], false, false);
            lo[i] = r2[0]; hi[i] = r2[1];
        }
        pb[X][sub][0] = __builtin_bit_cast(h8, lo);
        pb[X][sub][1] = __builtin_bit_cast(h8, hi);
    }
    template <bool OFF>                                      // OFF: the ablation without V^T P^T MFMAs
    __device__ __forceinline__ void mma(int X, int sub, int i) {
        const int t = i / 2, qg = i & 1;
        if constexpr (OFF) { asm volatile("" : "+v"(oacc[X][t][qg]) : "v"(vf[t][sub]), "v"(pb[X][sub][qg])); return; }
        oacc[X][t][qg] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf[t][sub], pb[X][sub][qg], oacc[X][t][qg], 0, 0, 0);
    }
    __device__ __forceinline__ void rescale(int X, float alpha) {
#pragma unroll
        for (int qg = 0; qg < 2; ++qg) {                     // O^T keeps query 16 qg + n16 on this lane: fetch ITS factor
            const float aq = __shfl(alpha, 16 * qg + n16);
#pragma unroll
            for (int t = 0; t < DT; ++t) oacc[X][t][qg] *= aq;
        }
    }
    // O = O^T / l: row D of O^T (tile D / 16, row D % 16: lane group (D % 16) / 4, register D % 4) is the denominator
    __device__ __forceinline__ void store(half_t* __restrict__ O, int ldo, size_t row0, int col0) {
        constexpr int LT = D / 16, LG = (D % 16) / 4, LR = D % 4;
#pragma unroll
        for (int X = 0; X < 2; ++X)
#pragma unroll
            for (int qg = 0; qg < 2; ++qg) {
                const float l = __shfl(oacc[X][LT][qg][LR], 16 * LG + n16);
                const float inv = 1.0f / l;
                half_t* op = O + (row0 + 32 * X + 16 * qg + n16) * ldo + col0;
#pragma unroll
                for (int t = 0; t < DT; ++t) {
                    const int dd = 16 * t + 4 * g;
                    if (dd < D) {
                        const h4 o4 = {(half_t)(oacc[X][t][qg][0] * inv), (half_t)(oacc[X][t][qg][1] * inv),
                                       (half_t)(oacc[X][t][qg][2] * inv), (half_t)(oacc[X][t][qg][3] * inv)};
                        *(h4*)(op + dd) = o4;
                    }
                }
            }
    }
};

template <int D>
struct Pv32 {
    static constexpr int DT = (D + 32) / 32;                 // 32-row tiles of O^T; row D carries the softmax denominator
    static constexpr int VBYTES = DT * 32 * 128, MIN_BLOCKS = D <= 40 ? 2 : 1, C_ZERO = 16;
    static constexpr int NPV = DT * 2, NRD = 2 * NPV, RD_B = NPV;      // the fragments of the first 32 keys in stage (b), the others in (c)
    static constexpr int MAXB0 = NPV - 3, MAXB1 = NPV - 2, MAXBX = NPV - 1;
    // LDS row rho = 8 a + 4 b + c holds key 16 (a >> 1) + 8 b + 4 (a & 1) + c: lane half b of the B operand of k-step s2 = a >> 1
    // holds the probabilities of LDS rows {8 (2 s2) + 4 b + c, 8 (2 s2 + 1) + 4 b + c}, i.e. of keys 16 s2 + 8 b + [0, 8)
    static __device__ __forceinline__ int key_of_row(int rho) {
        const int a = rho >> 3;
        return 16 * (a >> 1) + 8 * ((rho >> 2) & 1) + 4 * (a & 1) + (rho & 3);
    }
    // constant parts of the LDS image: rows D .. 32 DT - 1 of every slot's V^T (row D = ones), and [1 0 0 0 0 0 0 0] / zeros for
    // the fold slot of K
    static __device__ __forceinline__ void init_lds(char* smem, char* cst, int slots, int slot_bytes, int kbytes, int tid) {
        if (tid < 2) {
            h8 v = (h8)(half_t)0;
            if (tid == 0) v[0] = (half_t)1;
            *(h8*)(cst + tid * 16) = v;
        }
        for (int i = tid; i < slots * (DT * 32 - D) * 8; i += ATT_TS_Q) {
            const int sl_i = i / ((DT * 32 - D) * 8), rem = i - sl_i * ((DT * 32 - D) * 8), row = D + rem / 8, pc = rem & 7;
            *(h8*)(smem + sl_i * slot_bytes + kbytes + row * 128 + pc * 16) = row == D ? (h8)(half_t)1 : (h8)(half_t)0;
        }
    }

    int n32, h;                                              // query (O^T) / row (fragments) on lane & 31, half on lane >> 5
    int v_lane[2][2];                                        // V^T: row 32 t + n32, source piece 4 sub + 2 s2 + h at position (that) ^ ((n32 >> 1) & 7)
    h8 vf[DT][2][2], pf[2][2][2];
    f32x16 oacc[2][DT];
    __device__ __forceinline__ Pv32(int lane, int kbytes, const char* cst) : n32(lane & 31), h(lane >> 5) {
#pragma unroll
        for (int X = 0; X < 2; ++X)
#pragma unroll
            for (int t = 0; t < DT; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) oacc[X][t][r] = 0.f;
#pragma unroll
        for (int sub = 0; sub < 2; ++sub)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) v_lane[sub][s2] = kbytes + n32 * 128 + (((4 * sub + 2 * s2 + h) ^ ((n32 >> 1) & 7)) * 16);
    }
    __device__ __forceinline__ void rd_v(const char* sl, int n) {
        const int sub = n / NPV, t = (n % NPV) / 2, s2 = n & 1;
        vf[t][sub][s2] = *(const h8*)(sl + v_lane[sub][s2] + t * 32 * 128);
    }
    __device__ __forceinline__ void pack(int X, int sub, const f32x16& s) {      // registers 8 s2 .. 8 s2 + 7 are k-step s2's B operand
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
            for (int e = 0; e < 8; ++e) pf[X][sub][s2][e] = (half_t)s[8 * s2 + e];
    }
    template <bool OFF>
    __device__ __forceinline__ void mma(int X, int sub, int i) {
        const int t = i / 2, s2 = i & 1;
        if constexpr (OFF) { asm volatile("" : "+v"(oacc[X][t]) : "v"(vf[t][sub][s2]), "v"(pf[X][sub][s2])); return; }
        oacc[X][t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf[t][sub][s2], pf[X][sub][s2], oacc[X][t], 0, 0, 0);
    }
    __device__ __forceinline__ void rescale(int X, float alpha) {
#pragma unroll
        for (int t = 0; t < DT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) oacc[X][t][r] *= alpha;
    }
    // O = O^T / l: row D of O^T lives in tile D / 32, register ((D % 32) & 3) + 4 ((D % 32) >> 3) of the half with 4 h == (D % 32) & 4
    __device__ __forceinline__ void store(half_t* __restrict__ O, int ldo, size_t row0, int col0) {
        constexpr int rr = D % 32, reg = (rr & 3) + 4 * (rr >> 3), owner_half = (rr >> 2) & 1;
#pragma unroll
        for (int X = 0; X < 2; ++X) {
            const float mine = oacc[X][D / 32][reg];
            const float other = __shfl_xor(mine, 32);
            const float inv = 1.0f / (h == owner_half ? mine : other);
            half_t* op = O + (row0 + 32 * X + n32) * ldo + col0;
#pragma unroll
            for (int t = 0; t < DT; ++t)
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4) {
                    const int dd = t * 32 + 8 * g4 + 4 * h;
                    if (dd < D) {
                        const h4 o4 = {(half_t)(oacc[X][t][4 * g4] * inv), (half_t)(oacc[X][t][4 * g4 + 1] * inv),
                                       (half_t)(oacc[X][t][4 * g4 + 2] * inv), (half_t)(oacc[X][t][4 * g4 + 3] * inv)};
                        *(h4*)(op + dd) = o4;
                    }
                }
        }
    }
};

// ABL: ablation switches for tools/bench_attention.py (FGDM_ATTN_ABL; results are then meaningless): 1 = no exponentials,
// 2 = no maximum / offset decision, 4 = no LDS-DMA after the first two tiles, 16 = no V^T P^T MFMAs, 32 = no K Q^T MFMAs
template <int D, class PV, int ABL = 0>
__global__ __launch_bounds__(ATT_TS_Q, PV::MIN_BLOCKS) void attn_two_strand_kernel(const half_t* __restrict__ Q, int ldq,
                                                                                 const half_t* __restrict__ K, int ldk,
                                                                                 const half_t* __restrict__ Vt, int ldvt,
                                                                                 half_t* __restrict__ O, int ldo,
                                                                                 int H, int T, int Tk, float sl2e) {
    constexpr int NW = ATT_TS_Q / 64;                        // waves
    constexpr int DP = (D + 16) / 16 * 16, NKS = DP / 16;    // contraction length of K Q^T incl. the fold slot; k-steps of 16
    constexpr int DC = D / 8;                                // 16-byte pieces per K row
    constexpr int PS = D / 16, PH = (D % 16) / 8;            // fragment / lane half of contraction slot D
    constexpr int KROW = DC * 16, KBYTES = 64 * KROW, VDATA = D * 128, SLOT = KBYTES + PV::VBYTES;
    constexpr int NSLOT = 3;
    constexpr int NDMA = (KBYTES + VDATA) / 1024, NI = (NDMA + NW - 1) / NW;   // 1 KiB LDS-DMA wave-instructions per tile; per wave
    constexpr int NPV = PV::NPV;                             // V^T P^T MFMAs per 32-key sub-tile and strand
    static_assert(KBYTES % 1024 == 0 && VDATA % 1024 == 0 && NDMA >= NW, "whole wave-instructions per image");
    static_assert(PV::RD_B <= 2 * NKS && PV::MAXBX < NPV, "the schedule facts fit the stages they ride in");
    // K row stride: 4 mod 8 dwords makes sixteen consecutive rows tile the banks (d = 40: 80-byte rows).  d = 80 (160-byte rows: rows
    // r and r + 8 would meet in the same banks): the 16-byte pieces of rows with (r >> 3) & 1 are ROTATED by ROT = 5 positions,
    // half a row, on the source side -- sixteen consecutive rows then tile the banks again
    // d = 64 (128-byte rows, exactly the V^T row: rows r and r + 2 would meet): the pieces are XOR-swizzled by (r >> 1) & 7 on the
    // source side, as those of V^T are -- a K fragment read has the very bank pattern of a V^T fragment read
    constexpr bool KXOR = KROW == 128;
    constexpr int ROT = (KXOR || (KROW / 4) % 8 == 4) ? 0 : DC / 2;
    static_assert(KXOR || ROT == 0 || ((KROW / 4) % 16 == 8 && DC % 2 == 0), "K row stride");
    __shared__ __attribute__((aligned(1024))) char smem[NSLOT * SLOT + 64];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n32 = lane & 31, h = lane >> 5;                // S^T layout: query on lane & 31, key half on lane >> 5
    const int nqb = T / ATT_TS_Q;
    const int logical = att_logical_block();
    const int qblk = logical % nqb, bh = logical / nqb;
    const int b = bh / H, head = bh - b * H;
    const int q0w = qblk * ATT_TS_Q + wave * 64;             // first query of this wave; strand X: q0w + 32 X + [0, 32)
    const int nt = Tk >> 6;

    char* const cst = smem + NSLOT * SLOT;
    PV::init_lds(smem, cst, NSLOT, SLOT, KBYTES, tid);

    // ---- LDS-DMA plan of this wave: wave-instruction j = wave + 4 u of a tile (a surplus one repeats the wave's previous piece:
    // same bytes to the same address).  K piece L = 64 j + lane: LDS row L / DC (row order inside a 32-key sub-tile:
    // PV::key_of_row), position L % DC (which source piece it holds: KXOR / ROT); V^T piece L: row L / 8, LDS position L % 8 holds
    // source piece (L % 8) ^ ((row >> 1) & 7).
    const half_t* Kb = K + (size_t)b * Tk * ldk + head * D;
    const half_t* Vb = Vt + ((size_t)b * H + head) * D * ldvt;
    unsigned voff[NI], ldst[NI];
    bool isk[NI];
#pragma unroll
    for (int u = 0; u < NI; ++u) {
        int j = wave + NW * u;
        if (j >= NDMA) j -= NW;
        isk[u] = j < KBYTES / 1024;
        ldst[u] = (unsigned)j * 1024u;
        if (isk[u]) {
            const int L = 64 * j + lane, rp = L / DC, c = L - rp * DC;
            const int rho = rp & 31, key = (rp & 32) + PV::key_of_row(rho);
            const int cs = KXOR ? (c ^ ((rho >> 1) & 7)) : ROT ? (c + DC - ROT * ((rho >> 3) & 1)) % DC : c;      // LDS position c of this row holds source piece cs
            voff[u] = (unsigned)(key * ldk + cs * 8) * 2u;
        } else {
            const int L = 64 * (j - KBYTES / 1024) + lane, d = L >> 3, x = L & 7;
            voff[u] = (unsigned)(d * ldvt + ((x ^ ((d >> 1) & 7)) * 8)) * 2u;
        }
    }
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) const void*)smem;
    auto issue = [&](int t, auto slotc) {                    // tile t -> slot t % NSLOT
        const char* kb = (const char*)(Kb + (size_t)t * 64 * ldk);
        const char* vb = (const char*)(Vb + t * 64);
        const unsigned base = lds0 + (unsigned)decltype(slotc)::value * SLOT;
#pragma unroll
        for (int u = 0; u < NI; ++u) att_dma16(voff[u], isk[u] ? kb : vb, base + ldst[u]);
    };
    issue(0, std::integral_constant<int, 0>{});
    if (nt > 1) issue(1, std::integral_constant<int, 1>{});

    // ---- Q^T fragments (B operand of K Q^T), pre-scaled; slot D will carry -max
    h8 qf[2][NKS];
#pragma unroll
    for (int X = 0; X < 2; ++X)
#pragma unroll
        for (int s = 0; s < NKS; ++s) {
            const int c = 16 * s + 8 * h;
            qf[X][s] = (h8)(half_t)0;
            if (c < D) qf[X][s] = *(const h8*)(Q + ((size_t)b * T + q0w + 32 * X + n32) * ldq + head * D + c);
#pragma unroll
            for (int e = 0; e < 8; ++e) qf[X][s][e] = (half_t)((float)qf[X][s][e] * sl2e);
        }
    PV pv(lane, KBYTES, cst);                                // O^T = 0; V^T fragment addresses inside a slot (the V^T image follows the K image)
    float m_run[2] = {0.f, 0.f};

    // ---- K fragment addresses inside a slot: row (32 sub + n32), piece 2 s + h (swizzled: KXOR / ROT) -> immediate offsets
    // 32 KROW sub; pieces >= DC are the constants (the fold slot's k_lane is never used)
    int k_lane[NKS];
#pragma unroll
    for (int s2 = 0; s2 < NKS; ++s2)
        k_lane[s2] = KXOR  ? n32 * KROW + (((2 * s2 + h) & 7) ^ ((n32 >> 1) & 7)) * 16
                     : ROT ? n32 * KROW + ((2 * s2 + h + ROT * ((n32 >> 3) & 1)) % DC) * 16
                           : n32 * KROW + h * 16 + s2 * 32;      // unswizzled: one register, the k-step is an immediate
    const char* const c_one = cst, *const c_zero = cst + PV::C_ZERO;

    f32x16 sacc[2][2];
    h8 kf[2][NKS];
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    auto rd_k = [&](const char* sl, int sub, int s) {
        const int ci0 = 2 * s;                               // piece index of lane half 0; half 1 reads ci0 + 1
        const char* p = sl + k_lane[s] + sub * 32 * KROW;
        if (ci0 + 1 >= DC) {                                 // some lanes read a constant piece
            const char* cp0 = ci0 < DC ? p : (ci0 == DC ? c_one : c_zero);
            const char* cp1 = ci0 + 1 == DC ? c_one : c_zero;
            p = h ? cp1 : cp0;
        }
        kf[sub][s] = *(const h8*)p;
    };
    auto qk = [&](int X, int sub, int s) {
        if constexpr ((ABL & 32) != 0) { if (s == 0) asm volatile("" : "=v"(sacc[X][sub])); return; }
        sacc[X][sub] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[sub][s], qf[X][s], s == 0 ? zero16 : sacc[X][sub], 0, 0, 0);
    };
    auto pvm = [&](int X, int sub, int i) { pv.template mma<(ABL & 16) != 0>(X, sub, i); };      // V^T P^T step i of a sub-tile
    auto max_part = [&](int X, int sub, float mx) {          // 8 v_max3 over one sub-tile's 16 scores of this lane
        if constexpr ((ABL & 2) != 0) return mx;
#pragma unroll
        for (int r = 0; r < 16; r += 2) mx = fmaxf(fmaxf(mx, sacc[X][sub][r]), sacc[X][sub][r + 1]);
        return mx;
    };
    // the offset moves only when some query of the strand outgrew it by more than 2^ATT_THR (or on the first tile)
    auto decide = [&](int X, float mx, bool first) {
        if constexpr ((ABL & 2) != 0) return;
        if (first || !__all(mx <= ATT_THR)) {
            const float m_new = first ? mx : m_run[X] + fmaxf(mx, 0.f);
            const float m_hat = (float)(half_t)m_new;        // exactly what Q[q][D] can hold
            const float delta = m_run[X] - m_hat;
            m_run[X] = m_hat;
            if (!first) pv.rescale(X, __builtin_amdgcn_exp2f(delta));
#pragma unroll
            for (int sub = 0; sub < 2; ++sub)
#pragma unroll
                for (int r = 0; r < 16; ++r) sacc[X][sub][r] += delta;   // this tile was taken against the old offset
            if (h == PH) qf[X][PS][0] = (half_t)(-m_hat);
        }
    };
    auto expo = [&](int X, int sub, int r0, int r1) {
#pragma unroll
        for (int r = r0; r < r1; ++r) sacc[X][sub][r] = (ABL & 1) ? sacc[X][sub][r] : __builtin_amdgcn_exp2f(sacc[X][sub][r]);
    };

    // one tile; the ring slot is a compile-time constant (the loop below is unrolled over the slots), so every fragment address is
    // a loop-invariant register plus an immediate
    auto tile = [&](int kt, auto slotc) {
        constexpr int slot = decltype(slotc)::value;
        // my pieces of tile kt landed (tile kt + 1 may fly), then everybody's: one barrier per tile; behind it nobody reads the
        // slot that tile kt + 2 goes to (the one of tile kt - 1) any more
        if (!(ABL & 4) && kt + 1 < nt) att_wait_vmcnt<NI>(); else att_wait_vmcnt<0>();
        __builtin_amdgcn_s_waitcnt(0xC07F);
        __builtin_amdgcn_s_barrier();
        if (!(ABL & 4) && kt + 2 < nt) issue(kt + 2, std::integral_constant<int, (slot + 2) % NSLOT>{});
        const char* sl = smem + slot * SLOT;
        const bool first = kt == 0;
#pragma unroll
        for (int sub = 0; sub < 2; ++sub)
#pragma unroll
            for (int s = 0; s < NKS; ++s) rd_k(sl, sub, s);
        ATT_SB();
        // (b) K Q^T of strand A; the first RD_B V^T fragments of the tile are requested between its MFMAs
#pragma unroll
        for (int sub = 0; sub < 2; ++sub)
#pragma unroll
            for (int s = 0; s < NKS; ++s) {
                const int i = sub * NKS + s;
                qk(0, sub, s);
                if (i < PV::RD_B) pv.rd_v(sl, i);
                ATT_SB();
            }
        // (c) K Q^T of strand B  |  strand A: maximum, decision, exp and pack of its first 32 keys
        float mx = sacc[0][0][0];                            // (sub-tile 0 first: its MFMAs retired three MFMAs ago)
        qk(1, 0, 0); mx = max_part(0, 0, mx); ATT_SB();
        qk(1, 0, 1); mx = max_part(0, 1, mx); ATT_SB();
        qk(1, 0, 2 % NKS); mx = att_max_cross(mx); ATT_SB();
#pragma unroll
        for (int s = 3; s < NKS; ++s) { qk(1, 0, s); ATT_SB(); }
        decide(0, mx, first);
        ATT_SB();
#pragma unroll
        for (int s = 0; s < NKS; ++s) {
            qk(1, 1, s);
            expo(0, 0, 16 * s / NKS, 16 * (s + 1) / NKS);
            if (PV::RD_B + s < PV::NRD) pv.rd_v(sl, PV::RD_B + s);      // ... and the remaining V^T fragments
            ATT_SB();
        }
#pragma unroll
        for (int n = PV::RD_B + NKS; n < PV::NRD; ++n) pv.rd_v(sl, n);
        pv.pack(0, 0, sacc[0][0]);
        ATT_SB();
        // (d) V^T P^T of strand A, first 32 keys  |  strand A: exp of its second 32 keys; strand B: maximum
        float mxb = sacc[1][0][0];
#pragma unroll
        for (int i = 0; i < NPV; ++i) {
            pvm(0, 0, i);
            expo(0, 1, 16 * i / NPV, 16 * (i + 1) / NPV);
            if (i == PV::MAXB0) mxb = max_part(1, 0, mxb);
            if (i == PV::MAXB1) mxb = max_part(1, 1, mxb);
            if (i == PV::MAXBX) mxb = att_max_cross(mxb);
            ATT_SB();
        }
        pv.pack(0, 1, sacc[0][1]);
        ATT_SB();
        decide(1, mxb, first);
        ATT_SB();
        // (e) V^T P^T of strand A, second 32 keys  |  strand B: exp and pack of its first 32 keys
#pragma unroll
        for (int i = 0; i < NPV; ++i) {
            pvm(0, 1, i);
            expo(1, 0, 16 * i / NPV, 16 * (i + 1) / NPV);
            ATT_SB();
        }
        pv.pack(1, 0, sacc[1][0]);
        ATT_SB();
        // (f) V^T P^T of strand B, first 32 keys  |  strand B: exp and pack of its second 32 keys
#pragma unroll
        for (int i = 0; i < NPV; ++i) {
            pvm(1, 0, i);
            expo(1, 1, 16 * i / NPV, 16 * (i + 1) / NPV);
            ATT_SB();
        }
        pv.pack(1, 1, sacc[1][1]);
        ATT_SB();
        // (g) V^T P^T of strand B, second 32 keys
#pragma unroll
        for (int i = 0; i < NPV; ++i) pvm(1, 1, i);
        ATT_SB();
    };
    for (int kt = 0; kt < nt; kt += NSLOT) {
        tile(kt, std::integral_constant<int, 0>{});
        if (kt + 1 < nt) tile(kt + 1, std::integral_constant<int, 1>{});
        if (kt + 2 < nt) tile(kt + 2, std::integral_constant<int, 2>{});
    }

    pv.store(O, ldo, (size_t)b * T + q0w, head * D);
}

// Which kernel attention_launch chose on its last successful call in this process (fgdm_debug_last_attention_kernel: the parity
// tests assert that a case reaches the kernel it was written for).  Host side only: one store of a plain int per launch.
enum AttnKernelId { ATT_KID_NONE = 0, ATT_KID_GENERAL = 1, ATT_KID_CROSS = 2, ATT_KID_CROSS_LONG = 3, ATT_KID_PP = 4, ATT_KID_DQ16 = 5,
                    ATT_KID_DQ32 = 6,
                    // the capturing instantiations (attention_capture_launch)
                    ATT_KID_GENERAL_CAP = 7, ATT_KID_CROSS_CAP = 8, ATT_KID_CROSS_LONG_CAP = 9 };
static int g_last_attn_kernel = ATT_KID_NONE;
int attention_last_kernel() { return g_last_attn_kernel; }
static int att_launched(int kid) {
    if (hipGetLastError() != hipSuccess) return FGDM_ERR_HIP;
    g_last_attn_kernel = kid;
    return FGDM_OK;
}

// ---- launch helpers.  AttnCall: what attention_launch was called with (sl2e: the factor the kernels multiply Q by)
struct AttnCall {
    const half_t* Q; int ldq;
    const half_t* K; int ldk;
    const half_t* Vt; int ldvt;
    half_t* O; int ldo;
    int B, H, T, Tk;
    float sl2e;
    hipStream_t s;
    float* cap = nullptr;      // the per-head planes of a capturing call, else NULL
};
template <auto Kernel, class... Extra>
static int att_launch(const AttnCall& c, dim3 grid, int threads, int lds, int kid, Extra... extra) {
    FGDM_LAUNCH(Kernel, grid, dim3(threads), lds, c.s, c.Q, c.ldq, c.K, c.ldk, c.Vt, c.ldvt, c.O, c.ldo, c.H, c.T, c.Tk, c.sl2e, extra...);
    return att_launched(kid);
}
// f(std::integral_constant<int, d>) for the head widths of the networks (320 ... 1280 channels over 8 heads: 40 / 80 / 160; a fixed
// head width, num_head_channels = 64: 5 ... 20 heads)
template <class F>
static int by_head_width(int d, F&& f) {
    switch (d) {
        case 40: return f(std::integral_constant<int, 40>{});
        case 64: return f(std::integral_constant<int, 64>{});
        case 80: return f(std::integral_constant<int, 80>{});
        case 160: return f(std::integral_constant<int, 160>{});
        default: return FGDM_ERR_ARG;
    }
}

template <int D>
static int launch_general(const AttnCall& c) {
    const dim3 grid(((c.T + 127) / 128) * c.H * c.B);
    if (c.cap) return att_launch<attn_kernel<D, float*>>(c, grid, 256, 0, ATT_KID_GENERAL_CAP, c.cap);
    return att_launch<attn_kernel<D>>(c, grid, 256, 0, ATT_KID_GENERAL);
}
template <int D>
static int launch_pp(const AttnCall& c) {
    return att_launch<attn_pp_kernel<D>>(c, dim3(((c.T + 255) / 256) * c.H * c.B), 512, 0, ATT_KID_PP);
}

// The two-strand kernel: whole ATT_TS_Q-query blocks, whole 64-key tiles and at least two of them, and a tile's K / V^T byte offsets
// (the 32-bit voffset of the LDS-DMA) below 2^31
static bool two_strand_ok(const AttnCall& c, int d) {
    return c.T % ATT_TS_Q == 0 && c.Tk % 64 == 0 && c.Tk >= 128 && (size_t)64 * c.ldk * 2 < (1u << 31) && (size_t)d * c.ldvt * 2 < (1u << 31);
}
template <auto Kernel>
static int launch_two_strand(const AttnCall& c, int kid) {
    return att_launch<Kernel>(c, dim3((c.T / ATT_TS_Q) * c.H * c.B), ATT_TS_Q, 0, kid);
}
// FGDM_ATTN_ABL (tools/bench_attention.py only; see ABL above): the d = 40 kernels with parts of their work removed
template <int ABL>
static int launch_ablation(const AttnCall& c, bool wide) {
    return wide ? launch_two_strand<attn_two_strand_kernel<40, Pv32<40>, ABL>>(c, ATT_KID_DQ32) : launch_two_strand<attn_two_strand_kernel<40, Pv16<40>, ABL>>(c, ATT_KID_DQ16);
}
static int launch_ablation_bits(const AttnCall& c, int abl, bool wide) {
    switch (abl) {
        case 1: return launch_ablation<1>(c, wide);
        case 2: return launch_ablation<2>(c, wide);
        case 3: return launch_ablation<3>(c, wide);
        case 4: return launch_ablation<4>(c, wide);
        case 7: return launch_ablation<7>(c, wide);
        case 16: return launch_ablation<16>(c, wide);
        case 32: return launch_ablation<32>(c, wide);
        case 48: return launch_ablation<48>(c, wide);
        case 51: return launch_ablation<51>(c, wide);
        default: return FGDM_ERR_ARG;
    }
}

// The key-resident text kernel with cpw query chunks per wave.  (d = 160, NS = 8) does not fit the 160 KB of a CU and is never built.
static_assert(attn_cross_lds(64, 3) <= 64 * 1024 && attn_cross_lds(64, 8) <= 160 * 1024, "d = 64: NS = 3 static, every NS form fits a CU's LDS");
static_assert(attn_cross_lds(160, 7) <= 160 * 1024 && attn_cross_lds(160, 8) > 160 * 1024, "d = 160: up to NS = 7");
template <int D, int NS>
static int launch_cross(const AttnCall& c, int cpw) {
    constexpr int lds = attn_cross_lds(D, NS), dyn = NS == 3 ? 0 : lds;      // NS = 3 keeps its LDS static
    if constexpr (lds > 160 * 1024) {
        return FGDM_ERR_ARG;
    } else {
        if ((c.Tk + 31) / 32 != NS || c.ldvt < NS * 32) return FGDM_ERR_ARG;      // the kernel's contract: it masks sub-tile NS - 1 only
        const dim3 grid(((c.T + 128 * cpw - 1) / (128 * cpw)) * c.H * c.B);
        if (c.cap) {
            constexpr auto kc = attn_cross_kernel<D, NS, float*>;
            if (dyn && fgdm_dyn_lds<kc>(dyn) != FGDM_OK) return FGDM_ERR_HIP;
            return att_launch<kc>(c, grid, 256, dyn, NS == 3 ? ATT_KID_CROSS_CAP : ATT_KID_CROSS_LONG_CAP, cpw, c.cap);
        }
        constexpr auto k = attn_cross_kernel<D, NS>;
        if (dyn && fgdm_dyn_lds<k>(dyn) != FGDM_OK) return FGDM_ERR_HIP;
        return att_launch<k>(c, grid, 256, dyn, NS == 3 ? ATT_KID_CROSS : ATT_KID_CROSS_LONG, cpw);
    }
}
template <int D>
static int launch_cross_ns(const AttnCall& c, int ns, int cpw) {
    switch (ns) {
        case 3: return launch_cross<D, 3>(c, cpw);
        case 4: return launch_cross<D, 4>(c, cpw);
        case 5: return launch_cross<D, 5>(c, cpw);
        case 6: return launch_cross<D, 6>(c, cpw);
        case 7: return launch_cross<D, 7>(c, cpw);
        case 8: return launch_cross<D, 8>(c, cpw);
        default: return FGDM_ERR_ARG;
    }
}

// The first condition that holds decides (tests/attention_dispatch.py states the same rules a second time); the knobs are read in
// this order, each when its condition is reached.
// cap: NULL, or the per-head planes of a capturing call (attention_capture_launch).  The rules are the same either way; a capturing
// call that they send to a kernel without a capturing instantiation (the long self-attention kernels) is FGDM_ERR_ARG.
static int attention_dispatch(const half_t* Q, int ldq, const half_t* K, int ldk, const half_t* Vt, int ldvt, half_t* O,
                              int ldo, int B, int H, int T, int Tk, int d, int q_prescaled, float* cap, hipStream_t s) {
    if (B <= 0 || H <= 0 || T <= 0 || Tk <= 0) return FGDM_ERR_ARG;
    if (ldvt < (Tk + 63) / 64 * 64 || (ldvt & 7) || (ldq & 7) || (ldk & 7) || (ldo & 3)) return FGDM_ERR_ARG;
    // q_prescaled: the to_q weights were packed with log2(e) d^-1/2 folded in (fgdm_finalize_weights), so Q arrives in the
    // log2 domain with ONE fp16 rounding; the kernels then multiply by exactly 1
    const float sl2e = q_prescaled ? 1.0f : 1.4426950408889634f / sqrtf((float)d);
    const AttnCall c{Q, ldq, K, ldk, Vt, ldvt, O, ldo, B, H, T, Tk, sl2e, s, cap};
    const bool pp_on = knob_once(KNOB_ATTN_PP) != 0;
    // long self-attention, d = 40: the two-strand kernels.  FGDM_ATTN_DQ: 0 = off, 1 = 16-wide V^T P^T (the faster one on random
    // operands), anything else = 32-wide (default 3: the faster one inside the network).  Under FGDM_ATTN_ABL the
    // ablated 32-wide kernel is taken at FGDM_ATTN_DQ=3 only, the ablated 16-wide one otherwise
    const int dq = knob_once(KNOB_ATTN_DQ);
    if (dq > 0 && d == 40 && two_strand_ok(c, d)) {
        if (cap) return FGDM_ERR_ARG;
        if (const int abl = knob_once(KNOB_ATTN_ABL)) return launch_ablation_bits(c, abl, dq == 3);
        return dq == 1 ? launch_two_strand<attn_two_strand_kernel<40, Pv16<40>>>(c, ATT_KID_DQ16) : launch_two_strand<attn_two_strand_kernel<40, Pv32<40>>>(c, ATT_KID_DQ32);
    }
    // d = 80: the 32-wide kernel at one wave per SIMD (its two strands need ~280 registers); FGDM_ATTN_DQ80=0 switches it off (A/B)
    const int dq80 = knob_once(KNOB_ATTN_DQ80);
    if (cap && ((dq80 > 0 && (d == 80 || d == 64) && two_strand_ok(c, d)) || (pp_on && T >= 256 && Tk >= 256 && (d == 40 || d == 64 || d == 80))))
        return FGDM_ERR_ARG;
    if (dq80 > 0 && d == 80 && two_strand_ok(c, d)) return launch_two_strand<attn_two_strand_kernel<80, Pv32<80>>>(c, ATT_KID_DQ32);
    // d = 64 (SD-2.x: a fixed head width): the 32-wide kernel as well, one wave per SIMD like d = 80 and behind the same switch --
    // FGDM_ATTN_DQ80=0 sends both to the ping-pong kernel (A/B; the measurement behind the default: profiles/attention_d64.txt)
    if (dq80 > 0 && d == 64 && two_strand_ok(c, d)) return launch_two_strand<attn_two_strand_kernel<64, Pv32<64>>>(c, ATT_KID_DQ32);
    // every other long shape at d = 40 / 64 / 80: the eight-wave ping-pong kernel (256 queries per workgroup); FGDM_ATTN_PP=0 switches it off (A/B)
    if (pp_on && T >= 256 && Tk >= 256 && (d == 40 || d == 64 || d == 80)) return d == 40 ? launch_pp<40>(c) : d == 64 ? launch_pp<64>(c) : launch_pp<80>(c);
    // one text part (64 < Tk <= 96, NS = 3): the key-resident kernel.  FGDM_ATTN_CROSS: query chunks per wave, 0 = off (A/B)
    const int cross = knob_once(KNOB_ATTN_CROSS);
    if (cross > 0 && Tk > 64 && Tk <= 96 && ldvt >= 96 && T >= 128)
        return by_head_width(d, [&](auto dc) { return launch_cross<decltype(dc)::value, 3>(c, std::min(cross, T / 128)); });
    // two or three text parts (96 < Tk <= 256): the same kernel with NS = ceil(Tk / 32) sub-tiles where NS * 32 <= ldvt and the LDS
    // fits.  FGDM_ATTN_CROSS_LONG: query chunks per wave, 0 = off (A/B).  Default 8: staging 154 - 256 keys costs as much traffic as
    // the Q + O rows of 4 chunks, and at T = 1024 eight chunks make one workgroup per (batch, head) (measured:
    // profiles/long_context_attention.txt; 4 chunks do not beat attn_kernel at d = 80)
    const int cross_long = knob_once(KNOB_ATTN_CROSS_LONG), ns = (Tk + 31) / 32;
    if (cross_long > 0 && Tk > 96 && Tk <= 256 && T >= 128 && ldvt >= ns * 32 && (d == 40 || d == 64 || d == 80 || (d == 160 && ns <= 7)))
        return by_head_width(d, [&](auto dc) { return launch_cross_ns<decltype(dc)::value>(c, ns, std::min(cross_long, T / 128)); });
    // everything else: the general kernel
    return by_head_width(d, [&](auto dc) { return launch_general<decltype(dc)::value>(c); });
}
int attention_launch(const half_t* Q, int ldq, const half_t* K, int ldk, const half_t* Vt, int ldvt, half_t* O,
                     int ldo, int B, int H, int T, int Tk, int d, int q_prescaled, hipStream_t s) {
    return attention_dispatch(Q, ldq, K, ldk, Vt, ldvt, O, ldo, B, H, T, Tk, d, q_prescaled, nullptr, s);
}

// =====================================================================================================================
// Cross-attention maps.  The head reduction is a second, small kernel: the capturing instantiations above write one probability
// plane per head, and this kernel sums a (row, query, token) element over the planes h = 0 .. H - 1 IN THAT ORDER, one thread per
// element -- no atomics, no order that depends on scheduling: two runs give the same bits.  It also does the bookkeeping of the
// engine's capture plan: rows [row0, row0 + rows) of the batch (a CFG half), the token columns tok[0 .. ntok) (NULL: all Tk, in
// order), and A += mean (accumulate) or A = mean.  A is fp32 [rows, T, ntok].
__global__ __launch_bounds__(256) void attn_maps_reduce_kernel(const float* __restrict__ P, float* __restrict__ A, int H, int T, int Tk,
                                                               int row0, const int* __restrict__ tok, int ntok, int accumulate, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int j = (int)(i % ntok);
    const size_t bt = i / ntok;
    const int t = (int)(bt % T), b = row0 + (int)(bt / T);
    const int k = tok ? tok[j] : j;
    float sum = 0.f;
    for (int h = 0; h < H; ++h) sum += P[(((size_t)b * H + h) * T + t) * Tk + k];
    const float v = sum / (float)H;
    A[i] = accumulate ? A[i] + v : v;
}
size_t attention_capture_plane_floats(int B, int H, int T, int Tk) { return (size_t)B * H * T * Tk; }
int attention_capture_launch(const half_t* Q, int ldq, const half_t* K, int ldk, const half_t* Vt, int ldvt, half_t* O, int ldo,
                             int B, int H, int T, int Tk, int d, int q_prescaled, float* planes, hipStream_t s) {
    if (!planes || Tk > ATT_CAP_MAX_KEYS) return FGDM_ERR_ARG;
    return attention_dispatch(Q, ldq, K, ldk, Vt, ldvt, O, ldo, B, H, T, Tk, d, q_prescaled, planes, s);
}
int attention_maps_reduce(const float* planes, float* maps, int H, int T, int Tk, int row0, int rows, const int* tok, int ntok,
                          int accumulate, hipStream_t s) {
    if (!planes || !maps || H <= 0 || T <= 0 || Tk <= 0 || row0 < 0 || rows <= 0 || ntok <= 0 || (!tok && ntok != Tk)) return FGDM_ERR_ARG;
    const size_t n = (size_t)rows * T * ntok;
    FGDM_LAUNCH(attn_maps_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, planes, maps, H, T, Tk, row0, tok, ntok, accumulate, n);
    return hipGetLastError() == hipSuccess ? FGDM_OK : FGDM_ERR_HIP;
}
