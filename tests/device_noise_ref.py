"""TEST INFRASTRUCTURE shared by tests/test_device_noise_host.py (CPU) and tests/test_gpu_device_noise.py (GPU): the generator of
the armed device loops (fgdm_loop_noise_set, include/fgdm.h) restated in numpy from its description -- Philox4x32-10 from the round
function, the counter layout, and Box-Muller in float64.  Never imported by the product."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57                # the round's multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85                # the key schedule's increments
MASK = np.uint64(0xFFFFFFFF)
STREAM_STEP, STREAM_Q = 0, 1


def philox4x32_10(counter, key):
    """counter: four equal-shaped arrays (or ints) of 32-bit words, key: two 32-bit ints -> four uint32 arrays.  One round:
    (c0, c1, c2, c3) -> (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)); the key grows by (W0, W1) between rounds."""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in np.broadcast_arrays(*counter)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]            # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def seed_key(seed):
    return int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF


def counter_blocks(base, n):
    """the 128-bit counter `base` (four words, lowest first) + k for k in range(n), as four word arrays"""
    v = sum(int(w) << (32 * i) for i, w in enumerate(base))
    vals = [(v + k) % (1 << 128) for k in range(n)]
    return [np.array([(x >> (32 * i)) & 0xFFFFFFFF for x in vals], dtype=np.uint64) for i in range(4)]


def words(seed, stream, step, B, per_sample, first_sample=0, repeat=False):
    """uint32 [B, per_sample / 4, 4]: the generator's output block of every four elements of every row"""
    assert per_sample % 4 == 0
    q = np.arange(per_sample // 4, dtype=np.uint64)[None, :]
    sample = (np.zeros(B, dtype=np.uint64) if repeat else np.arange(first_sample, first_sample + B, dtype=np.uint64))[:, None]
    return np.stack(philox4x32_10((q, sample, step, stream), seed_key(seed)), axis=-1)


def box_muller64(w):
    """float64 [..., 4] from uint32 [..., 4]: (r0, r1) -> (rho cos, rho sin), (r2, r3) likewise, exactly as described"""
    w = w.astype(np.uint64)
    u1 = ((w[..., 0::2] >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
    u2 = (w[..., 1::2] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    rho = np.sqrt(-2.0 * np.log(u1))
    # theta = 2 pi u2 with the quadrant taken off exactly (2 u2 is a multiple of 2^-23), so that the reference is good to a
    # float64 rounding RELATIVE to the value also next to the zeros of cos and sin, where pi's own rounding would show
    t = 2.0 * u2
    n = np.floor(2.0 * t + 0.5)
    r = t - 0.5 * n                                                     # exact, in [-1/4, 1/4]
    s, c = np.sin(np.pi * r), np.cos(np.pi * r)
    n = n.astype(np.int64) % 4
    cos = np.choose(n, [c, -s, -c, s])
    sin = np.choose(n, [s, c, -s, -c])
    return np.stack([rho * cos, rho * sin], axis=-1).reshape(*w.shape[:-1], 4)


def randn64(seed, stream, step, B, per_sample, first_sample=0, repeat=False):
    """float64 [B, per_sample]: the exact normals behind fgdm_randn at temperature 1"""
    return box_muller64(words(seed, stream, step, B, per_sample, first_sample, repeat)).reshape(B, per_sample)
