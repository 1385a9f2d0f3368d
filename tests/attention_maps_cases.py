"""Cases, operands and references of tests/test_gpu_attention_maps.py, shared with tools/attention_maps_bound.py (which measures
the bound on the CPU and writes profiles/attention_maps_parity_errors.txt).

All cases run with q_prescaled = 1, the mode the engine calls the kernels in: Q' = fp16(q log2(e) d^-1/2) arrives and the maps are
softmax_2(Q' K^T) = exp2(s - max) / sum, so the float64 reference sees exactly the operands the kernel sees.  (Without the flag the
d = 40 kernels round Q log2(e) d^-1/2 to fp16 themselves, an operand rounding of 2^-11 that no fp32 evaluation has; the test holds
that mode to the bit-equality of O and to the row sums only.)"""
import math

import torch

LOG2E = 1.4426950408889634
# (B, heads, T, Tk, d, layout): T = 64 reaches the general kernel, 256 the key-resident ones in whole chunks, 200 leaves the last
# 128-query block and its last 32-query chunk ragged; B = 1 is every sample of a B = 3 case run on its own
CASES = [(3, Hh, T, Tk, d, 'compact') for d in (40, 64, 80, 160) for Hh in (5, 8) for T in (64, 200, 256) for Tk in (77, 154)]
CASES += [(3, 5, 200, Tk, d, 'all_different') for d in (40, 64, 80, 160) for Tk in (77, 154)]
MARGIN = 4.0


def case_id(c):
    return f'B{c[0]}H{c[1]}T{c[2]}Tk{c[3]}d{c[4]}_{c[5]}'


def inputs(case):
    """unit randn operands, one key spiked against query 0 of head 0; Q already pre-scaled and rounded to fp16"""
    B, Hh, T, Tk, d, _ = case
    Cc = Hh * d
    g = torch.Generator().manual_seed(1000 + 7 * T + Tk + d + Hh)
    q, k, v = (torch.randn(B, n, Cc, generator=g).half().float() for n in (T, Tk, Tk))
    k[:, 70, :d] = q[:, 0, :d] * 4.0
    qs = (q.double() * (LOG2E / math.sqrt(d))).half().float()
    return qs, k, v


def maps_reference(qs, k, B, Hh, d, dtype=torch.float64):
    """mean over heads of softmax_2(Q' K^T) in `dtype`, from the fp16-rounded operands: [B, T, Tk]"""
    qh = qs.view(B, -1, Hh, d).permute(0, 2, 1, 3).to(dtype)
    kh = k.view(B, -1, Hh, d).permute(0, 2, 1, 3).to(dtype)
    s = torch.matmul(qh, kh.transpose(-1, -2))
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    return (p / p.sum(-1, keepdim=True)).mean(1)


def relerr(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def measure_bound():
    """(per-case errors of the plain fp32 evaluation against float64, worst, bound = MARGIN * worst)"""
    errs = []
    for c in CASES:
        qs, k, _ = inputs(c)
        errs.append(relerr(maps_reference(qs, k, c[0], c[1], c[4], torch.float32), maps_reference(qs, k, c[0], c[1], c[4])))
    worst = max(errs)
    return errs, worst, MARGIN * worst
