"""The cases of tests/test_gpu_two_strand_bits.py and tools/record_two_strand_bits.py: the two-strand attention kernels of
fgdm_amd/csrc/attention.hip under the engine's call, small enough to launch all 64 in a few seconds, hashed instead of stored.

  kernels   32-wide V^T P^T at d = 40, 64, 80 (the defaults) and 16-wide at d = 40 (FGDM_ATTN_DQ=1, read once per process: those
            cases run in a fresh interpreter, `python tests/two_strand_bits_cases.py w16`, which prints their hashes as JSON)
  shapes    (B, H, T, Tk): two tiles (the shortest ring), three (every slot once), four (slot 0 refilled; two query blocks per
            (batch, head)), seven (the loop tail ends on slot 0)
  strides   Q and K are column blocks of stacked q|k|v rows (ldq = ldk = 3 H d); V^T rows hold the keys plus 64 (NaN: never read)
  scale     q_prescaled 0 and 1
  regimes   'ordinary' (unit-normal operands) and 'climb_9' (regime_inputs of tests/test_gpu_attention_calls.py: every row's logits
            rise by 9 log2 units per 64-key tile, so the offset decision rescales O on every tile after the first;
            rescaled_tiles() below shows it on the CPU)

Inputs come from numpy.random.default_rng seeded by the case, so they are the same bytes everywhere; their hash is recorded next
to the output's, and a replay that fails on the INPUT hash says that the generator moved, not the kernel."""
import ctypes as C
import hashlib
import json
import math
import os
import subprocess
import sys

import numpy as np

LOG2E = 1.4426950408889634
TWO_STRAND_16, TWO_STRAND_32 = 5, 6       # fgdm_debug_last_attention_kernel (include/fgdm.h)
KERNELS = (('w32', 40), ('w32', 64), ('w32', 80), ('w16', 40))
KERNEL_IDS = {'w32': TWO_STRAND_32, 'w16': TWO_STRAND_16}
SHAPES = ((2, 2, 256, 128), (2, 3, 256, 192), (2, 2, 512, 256), (2, 2, 256, 448))
REGIMES = ('ordinary', 'climb_9')
CLIMB_Q, CLIMB_NOISE, CLIMB_RATE = 4.0, 0.5, 9.0       # as in tests/test_gpu_attention_calls.py
CASES = [(w, d, shape, regime, pre) for w, d in KERNELS for shape in SHAPES for regime in REGIMES for pre in (0, 1)]


def case_id(case):
    w, d, (B, H, T, Tk), regime, pre = case
    return f'{w}_d{d}_B{B}H{H}T{T}Tk{Tk}_{regime}_{"prescaled" if pre else "scaled"}'


def operands(case):
    """(q [B, T, C], k [B, Tk, C], v [B, Tk, C]) fp16, Q as the call receives it (already in the log2 domain when pre-scaled)"""
    w, d, (B, H, T, Tk), regime, pre = case
    Cc = H * d
    rng = np.random.default_rng([d, B, H, T, Tk, REGIMES.index(regime)])
    q, k, v = (rng.standard_normal(s, dtype=np.float32) for s in ((B, T, Cc), (B, Tk, Cc), (B, Tk, Cc)))
    if regime == 'climb_9':
        u = np.full(d, d ** -0.5, dtype=np.float32)
        qh = (q * CLIMB_NOISE).reshape(B, T, H, d)
        q = (qh - (qh * u).sum(-1, keepdims=True) * u).reshape(B, T, Cc) + np.tile(CLIMB_Q * u, H)
        cj = (CLIMB_RATE * np.arange(Tk, dtype=np.float32) / 64.0) * (math.sqrt(d) / LOG2E) / CLIMB_Q
        k = k * CLIMB_NOISE + cj.reshape(1, Tk, 1) * np.tile(u, H)
    q = q.astype(np.float16)
    if pre:
        q = (q.astype(np.float64) * (LOG2E / math.sqrt(d))).astype(np.float16)
    return q, k.astype(np.float16), v.astype(np.float16)


def buffers(case):
    """the three device images of the call: Q rows [B T, 3 C] with Q in columns [0, C), K rows [B Tk, 3 C] with K in columns
    [C, 2 C) (the other column blocks hold the other operands, as the stacked projection leaves them), V^T [B, C, Tk + 64]"""
    w, d, (B, H, T, Tk), regime, pre = case
    Cc = H * d
    q, k, v = operands(case)
    qrows = np.concatenate([q.reshape(B * T, Cc), q.reshape(B * T, Cc)[::-1], -q.reshape(B * T, Cc)], 1)
    krows = np.concatenate([v.reshape(B * Tk, Cc), k.reshape(B * Tk, Cc), v.reshape(B * Tk, Cc)], 1)
    vt = np.full((B, Cc, Tk + 64), np.nan, dtype=np.float16)
    vt[:, :, :Tk] = v.transpose(0, 2, 1)
    return np.ascontiguousarray(qrows), np.ascontiguousarray(krows), vt


def rescaled_tiles(case):
    """CPU emulation of the kernels' offset decision (decide() in attention.hip): per 32-query strand, the tiles kt >= 1 on which
    some query's tile maximum exceeds the running offset by more than 2^8, which is where O is rescaled.  Returns a bool array
    [B, H, T / 32, Tk / 64 - 1]."""
    w, d, (B, H, T, Tk), regime, pre = case
    q, k, _ = operands(case)
    if not pre:
        q = (q.astype(np.float32) * np.float32(LOG2E / math.sqrt(d))).astype(np.float16)
    qh = q.astype(np.float64).reshape(B, T, H, d).transpose(0, 2, 1, 3)
    kh = k.astype(np.float64).reshape(B, Tk, H, d).transpose(0, 2, 3, 1)
    tmax = (qh @ kh).reshape(B, H, T // 32, 32, Tk // 64, 64).max(-1)       # [B, H, strand, query, tile]
    m = tmax[..., 0].astype(np.float16).astype(np.float64)
    took = np.zeros((B, H, T // 32, Tk // 64 - 1), dtype=bool)
    for kt in range(1, Tk // 64):
        mx = tmax[..., kt] - m
        move = (mx > 8.0).any(-1)
        m = np.where(move[..., None], (m + np.maximum(mx, 0.0)).astype(np.float16).astype(np.float64), m)
        took[..., kt - 1] = move
    return took


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def run(lib, case):
    """one call through fgdm_op_attention (q_prescaled 0) / fgdm_op_attention_ex (1); returns {'kernel', 'in', 'out'}"""
    import torch
    w, d, (B, H, T, Tk), regime, pre = case
    Cc = H * d
    host = buffers(case)
    qd, kd, vtd = (torch.from_numpy(a).cuda() for a in host)
    out = torch.full((B * T, Cc), float('nan'), dtype=torch.half, device='cuda')
    p = lambda addr: C.c_void_p(int(addr))
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    args = (p(qd.data_ptr()), 3 * Cc, p(kd.data_ptr() + 2 * Cc), 3 * Cc, p(vtd.data_ptr()), Tk + 64, p(out.data_ptr()), Cc, B, H, T, Tk, d)
    rc = lib.fgdm_op_attention_ex(*args, 1, st) if pre else lib.fgdm_op_attention(*args, st)
    assert rc == 0, (case_id(case), rc)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()), f'{case_id(case)}: an output element is NaN (unwritten, or a NaN pad was read) or infinite'
    return {'kernel': lib.fgdm_debug_last_attention_kernel(), 'in': sha(*host), 'out': sha(out.cpu().numpy())}


def run_width(lib, width):
    return {case_id(c): run(lib, c) for c in CASES if c[0] == width}


def run_16_wide():
    """the w16 cases in a fresh interpreter under FGDM_ATTN_DQ=1 (the knob is read once per process)"""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), 'w16'], env=dict(os.environ, FGDM_ATTN_DQ='1'),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    line = [ln for ln in r.stdout.splitlines() if ln.startswith('TWO_STRAND_BITS ')]
    assert len(line) == 1, r.stdout[-2000:]
    return json.loads(line[0][len('TWO_STRAND_BITS '):])


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from fgdm_amd import _lib
    print('TWO_STRAND_BITS ' + json.dumps(run_width(_lib.load(), sys.argv[1])))
