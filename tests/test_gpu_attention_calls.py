"""The attention kernels under the call the ENGINE makes, not only under the shapes it makes it with.

tests/test_gpu_ops.py and tests/test_gpu_long_context.py cover the shapes of the five kernels of fgdm_amd/csrc/attention.hip with
compact buffers (ldq == ldk == ldo == heads * d), the unscaled-Q mode and unit-normal operands.  The engine calls them with Q and K
as column halves of one [B T, 2 C] buffer (ldq = ldk = 2 C, ldo = C), with Q already in the log2 domain (q_prescaled = 1: the
kernels scale by exactly 1) and with whatever logits the network produces.  Here:

  KERNEL_CASES   one table; every case names the kernel it must reach and asserts fgdm_debug_last_attention_kernel() after its
                 call, and every instantiation attention_launch launches by default is reached (test_every_instantiation_has_a_case).
  B1 layouts     the engine's self-attention layout, three different leading dimensions with NaN row gaps, a wide V^T with NaN
                 beyond roundup(Tk, 64); bitwise equal to the compact call, nothing stored between output rows.
  B2 pre-scaled  fgdm_op_attention_ex(q_prescaled = 1) against softmax(ln 2 Q' K^T) V.
  B3 regimes     large / all-negative / flat / mixed rows / climbing and falling / late maximum / dominant key logits on every
                 kernel in both scale modes, judged against the family bar or 1.5 x the error of a CPU emulation of the kernels'
                 documented rounding policy, whichever is larger.
  B4             small_attn_kernel (the text encoder's causal attention) on its own.

Every output is a guarded, poisoned buffer (tests/guarded.py); every reference is float64 on the CPU from the fp16-rounded operands
and reads nothing a kernel produced."""
import ctypes as C
import math
import os
import subprocess
import sys

import pytest
import torch

import attention_dispatch as AD
from common import relerr
from guarded import LOCAL_TOL, guarded_in, guarded_out, tile_err
from test_gpu_long_context import spike_keys
from test_gpu_ops import TOL, close, din, h16, rnd, _st

pytestmark = pytest.mark.gpu

LOG2E = 1.4426950408889634
NAN16 = float('nan')


@pytest.fixture(scope='module')
def lib():
    from fgdm_amd import _lib
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return _lib.load()


def vp(addr):
    return C.c_void_p(int(addr))


# ------------------------------------------------------------------------------------------------------------- the cases
# (kernel, B, heads, T, Tk, d, regimes): the conditions are those of attention_launch today.  B >= 2 and heads >= 2 everywhere,
# so batch and head offsets are multiplied by the strides too.  `regimes` False: the case is too large for the many CPU
# references of B3 (the T = 4096 self-attention cases; their kernels have smaller cases there).
def _c(kernel, B, H, T, Tk, d, regimes=True):
    return (kernel, B, H, T, Tk, d, regimes)


KERNEL_CASES = [
    # general attn_kernel: Tk <= 64, or T < 128, or d = 160 self-attention, or d = 160 with eight 32-key sub-tiles
    _c(AD.GENERAL, 2, 2, 64, 64, 40), _c(AD.GENERAL, 2, 2, 100, 333, 40), _c(AD.GENERAL, 2, 3, 100, 130, 80),
    _c(AD.GENERAL, 2, 2, 192, 64, 80), _c(AD.GENERAL, 2, 2, 256, 256, 160), _c(AD.GENERAL, 2, 3, 200, 321, 160),
    _c(AD.GENERAL, 2, 2, 300, 250, 160),
    # text-token attn_cross_kernel<D, 3> (64 < Tk <= 96, T >= 128): one and several chunks per wave, ragged T, both key-count limits
    _c(AD.TEXT_TOKEN, 2, 2, 128, 77, 40), _c(AD.TEXT_TOKEN, 2, 3, 700, 65, 40), _c(AD.TEXT_TOKEN, 2, 2, 1024, 77, 80),
    _c(AD.TEXT_TOKEN, 3, 2, 130, 96, 80), _c(AD.TEXT_TOKEN, 2, 2, 512, 77, 160), _c(AD.TEXT_TOKEN, 2, 2, 700, 96, 160),
    # long-text attn_cross_kernel<D, NS> (96 < Tk <= 256, T >= 128): NS = ceil(Tk / 32) = 4 ... 8 (d = 160: 4 ... 7)
    _c(AD.LONG_TEXT, 2, 2, 128, 97, 40), _c(AD.LONG_TEXT, 2, 2, 700, 129, 40), _c(AD.LONG_TEXT, 2, 3, 1024, 161, 40),
    _c(AD.LONG_TEXT, 2, 2, 300, 200, 40), _c(AD.LONG_TEXT, 2, 2, 130, 231, 40),
    _c(AD.LONG_TEXT, 2, 2, 700, 128, 80), _c(AD.LONG_TEXT, 2, 2, 128, 154, 80), _c(AD.LONG_TEXT, 2, 2, 300, 192, 80),
    _c(AD.LONG_TEXT, 2, 3, 130, 193, 80), _c(AD.LONG_TEXT, 2, 2, 1000, 255, 80),
    _c(AD.LONG_TEXT, 2, 2, 300, 97, 160), _c(AD.LONG_TEXT, 2, 2, 128, 160, 160), _c(AD.LONG_TEXT, 2, 2, 700, 161, 160),
    _c(AD.LONG_TEXT, 2, 2, 130, 224, 160),
    # ping-pong attn_pp_kernel: T, Tk >= 256 with T % 256 != 0 or Tk % 64 != 0
    _c(AD.PING_PONG, 2, 2, 320, 320, 40), _c(AD.PING_PONG, 2, 2, 512, 257, 40), _c(AD.PING_PONG, 2, 2, 384, 300, 80),
    _c(AD.PING_PONG, 2, 2, 256, 321, 80),
    # two-strand 32-wide attn_dq32_kernel: T % 256 == 0, Tk % 64 == 0, Tk >= 128 (also T != Tk); under FGDM_ATTN_DQ=1 the d = 40
    # cases reach the 16-wide attn_dq_kernel (test_two_strand_16_wide_kernel_under_its_knob)
    _c(AD.TWO_STRAND_32, 2, 2, 4096, 4096, 40, False), _c(AD.TWO_STRAND_32, 2, 2, 512, 512, 40),
    _c(AD.TWO_STRAND_32, 2, 2, 256, 1024, 40), _c(AD.TWO_STRAND_32, 2, 3, 256, 128, 40),
    _c(AD.TWO_STRAND_32, 2, 2, 4096, 4096, 80, False), _c(AD.TWO_STRAND_32, 2, 2, 512, 512, 80),
    _c(AD.TWO_STRAND_32, 2, 2, 256, 320, 80),
]


def case_id(c):
    return f'{AD.KERNEL_NAMES[c[0]]}_d{c[5]}_B{c[1]}H{c[2]}T{c[3]}Tk{c[4]}'


REGIME_CASES = [c for c in KERNEL_CASES if c[6]]


def want_kernel(case):
    """the table's kernel; under FGDM_ATTN_DQ=1 the d = 40 two-strand cases must reach the 16-wide kernel"""
    kernel, d = case[0], case[5]
    if kernel == AD.TWO_STRAND_32 and d == 40 and os.environ.get('FGDM_ATTN_DQ') == '1':
        return AD.TWO_STRAND_16
    return kernel


def assert_kernel(lib, case):
    kernel, B, Hh, T, Tk, d, _ = case
    want = want_kernel(case)
    got = lib.fgdm_debug_last_attention_kernel()
    assert got == want, f'{case_id(case)}: ran on kernel {got} ({AD.KERNEL_NAMES.get(got)}), the case is written for {AD.KERNEL_NAMES[want]}'
    assert AD.expected_kernel(T, Tk, d) == want, 'tests/attention_dispatch.py disagrees with the case table'


def test_every_instantiation_has_a_case():
    """every (kernel, head width[, NS]) attention_launch launches by default is named by at least one case"""
    seen = {(c[0], c[5]) + (((c[4] + 31) // 32,) if c[0] == AD.LONG_TEXT else ()) for c in KERNEL_CASES}
    want = {(k, d) for k in (AD.GENERAL, AD.TEXT_TOKEN) for d in (40, 80, 160)}
    want |= {(k, d) for k in (AD.PING_PONG, AD.TWO_STRAND_32) for d in (40, 80)}
    want |= {(AD.LONG_TEXT, d, ns) for d in (40, 80) for ns in range(4, 9)} | {(AD.LONG_TEXT, 160, ns) for ns in range(4, 8)}
    assert seen == want, seen ^ want
    for c in KERNEL_CASES:
        assert AD.expected_kernel(c[3], c[4], c[5], env={}) == c[0], case_id(c)
        assert c[1] >= 2 and c[2] >= 2
    for k in (AD.GENERAL, AD.TEXT_TOKEN, AD.LONG_TEXT, AD.PING_PONG, AD.TWO_STRAND_32):
        assert any(c[0] == k and c[6] for c in KERNEL_CASES), 'every kernel needs a case in the logit regimes'
        for d in {c[5] for c in KERNEL_CASES if c[0] == k}:
            assert any(c[0] == k and c[5] == d and c[6] for c in KERNEL_CASES), (k, d)


# ------------------------------------------------------------------------------------------------------- CPU references
def heads_of(t, B, Hh, d):
    return t.view(B, -1, Hh, d).permute(0, 2, 1, 3)


def rows_of(o, B, Hh, d):       # [B, H, T, d] -> [B T, H d]
    return o.permute(0, 2, 1, 3).reshape(-1, Hh * d)


def reference(q, k, v, B, Hh, d, scale2):
    """float64 softmax(ln 2 * scale2 * q k^T) v from the fp16-rounded operands; returns ([B T, C], logits in log2 units)"""
    s = torch.matmul(heads_of(q, B, Hh, d).double(), heads_of(k, B, Hh, d).double().transpose(-1, -2)) * scale2
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    o = torch.matmul(p, heads_of(v, B, Hh, d).double()) / p.sum(-1, keepdim=True)
    return rows_of(o, B, Hh, d), s


def emulate(q, k, v, B, Hh, d, prescaled):
    """The kernels' documented rounding policy on the CPU: Q times log2(e) d^-1/2 rounded to fp16 when it does not arrive
    pre-scaled, logits rounded to fp32, P = fp16(exp2(s - m)) with the EXACT row maximum, denominator = the sum of those fp16 P,
    output rounded to fp16; everything else float64."""
    if not prescaled:
        sl2e = torch.tensor(LOG2E / math.sqrt(d), dtype=torch.float32)
        q = (q.float() * sl2e).half().float()
    s = torch.matmul(heads_of(q, B, Hh, d).double(), heads_of(k, B, Hh, d).double().transpose(-1, -2)).float()
    p = torch.exp2((s - s.amax(-1, keepdim=True)).double()).half().double()
    o = torch.matmul(p, heads_of(v, B, Hh, d).double()) / p.sum(-1, keepdim=True)
    return rows_of(o, B, Hh, d).half().double()


def prescale(q, d):
    """Q' = fp16(q log2(e) / sqrt(d)) on the host, as the engine's to_q weights deliver it"""
    return (q.double() * (LOG2E / math.sqrt(d))).half().float()


# ------------------------------------------------------------------------------------------------------------- layouts
def strided_in(t2d, ld):
    """[rows, C] fp16 -> a device [rows, ld] buffer between NaN guards whose columns >= C are NaN; returns (buffer, its [:, :C])"""
    rows, Cc = t2d.shape
    full = torch.full((rows, ld), NAN16, dtype=torch.half)
    full[:, :Cc] = t2d
    buf = guarded_in(full)
    return buf


def make_vt(v, B, Tk, Cc, ldvt, beyond=0.0):
    """V^T [B, C, ldvt]: columns [Tk, roundup(Tk, 64)) ZERO (the contract of include/fgdm.h), columns beyond that `beyond`"""
    Tkp = (Tk + 63) // 64 * 64
    vt = torch.full((B, Cc, ldvt), beyond, dtype=torch.half)
    vt[:, :, :Tkp] = 0
    vt[:, :, :Tk] = v.permute(0, 2, 1).half()
    return vt


LAYOUTS = ('compact', 'engine_self', 'all_different', 'wide_vt')


def launch(lib, layout, q, k, v, case, prescaled=None):
    """one call in the given layout; returns (GuardedOut, its logical [B T, C] region index, keep-alive list).
    prescaled None: fgdm_op_attention; 0 / 1: fgdm_op_attention_ex with that flag"""
    _, B, Hh, T, Tk, d, _ = case
    Cc = Hh * d
    Tkp = (Tk + 63) // 64 * 64
    q2, k2 = q.reshape(B * T, Cc).half(), k.reshape(B * Tk, Cc).half()
    ldq = ldk = ldo = Cc
    ldvt, beyond = Tkp, 0.0
    if layout == 'engine_self':
        # ONE [B T, 2 C] buffer, Q = columns [0, C), K = columns [C, 2 C): attention_launch(qk.p, 2 C, qk.p + C, 2 C, ..., a.p, C, ...)
        assert T == Tk
        qk = din(torch.cat([q2, k2], 1))
        qp, kp, keep = qk.data_ptr(), qk.data_ptr() + 2 * Cc, [qk]
        ldq = ldk = 2 * Cc
    elif layout == 'all_different':
        # values that satisfy attention_launch's alignment checks (ldq & 7, ldk & 7, ldo & 3)
        ldq, ldk, ldo = Cc + 8, 2 * Cc + 16, Cc + 4
        qb, kb = strided_in(q2, ldq), strided_in(k2, ldk)
        qp, kp, keep = qb.data_ptr(), kb.data_ptr(), [qb, kb]
    else:
        qb, kb = din(q2), din(k2)
        qp, kp, keep = qb.data_ptr(), kb.data_ptr(), [qb, kb]
        if layout == 'wide_vt':
            # no kernel reads a V^T column >= roundup(Tk, 64) (they load whole 32- / 64-key tiles up to there): NaN
            ldvt, beyond = Tkp + 64, NAN16
    vtd = din(make_vt(v, B, Tk, Cc, ldvt, beyond))
    out = guarded_out((B * T, ldo), torch.half)
    args = (vp(qp), ldq, vp(kp), ldk, vp(vtd.data_ptr()), ldvt, vp(out.data_ptr()), ldo, B, Hh, T, Tk, d)
    if prescaled is None:
        rc = lib.fgdm_op_attention(*args, _st())
    else:
        rc = lib.fgdm_op_attention_ex(*args, int(prescaled), _st())
    assert rc == 0, (layout, rc)
    torch.cuda.synchronize()
    assert_kernel(lib, case)
    region = (slice(None), slice(0, Cc))
    out.check(region)
    if ldo > Cc:
        out.assert_untouched((slice(None), slice(Cc, ldo)))      # no kernel may write between rows
    keep.append(vtd)
    return out, region, keep


def unit_inputs(case, seeds=(41, 42, 43), spike=70):
    """the operands of test_attention: unit randn, one key spiked against query 0 of head 0"""
    _, B, Hh, T, Tk, d, _ = case
    Cc = Hh * d
    q, k, v = h16(rnd((B, T, Cc), seeds[0])), h16(rnd((B, Tk, Cc), seeds[1])), h16(rnd((B, Tk, Cc), seeds[2]))
    if spike is not None and Tk > spike:
        k[:, spike, :d] = q[:, 0, :d] * 4.0
    return q, k, v


# ------------------------------------------------------------------------------------------------------------ B1 layouts
@pytest.mark.parametrize('case', KERNEL_CASES, ids=case_id)
def test_attention_layouts(lib, case):
    """Bars: this family's own (test_attention): normwise < TOL, blockwise < 2 TOL over 32 x 32 blocks.  A layout changes only
    addresses, never arithmetic: each strided output equals the compact one bit for bit (no kernel here orders work by an address)."""
    _, B, Hh, T, Tk, d, _ = case
    Cc = Hh * d
    q, k, v = unit_inputs(case)
    ref, _ = reference(q, k, v, B, Hh, d, LOG2E / math.sqrt(d))
    compact = None
    for layout in LAYOUTS:
        if layout == 'engine_self' and T != Tk:
            continue
        out, region, keep = launch(lib, layout, q, k, v, case)
        got = out.t[region]
        what = f'attention layout {layout} {case_id(case)}'
        assert relerr(got.float().cpu(), ref) < TOL, what
        close(what, got, ref, local=2 * TOL)
        if compact is None:
            compact = got.clone()
        else:
            assert torch.equal(got, compact), f'{what}: differs from the compact-layout result of the same operands'


# -------------------------------------------------------------------------------------------------------- B2 pre-scaled Q
@pytest.mark.parametrize('case', KERNEL_CASES, ids=case_id)
def test_attention_prescaled_q(lib, case):
    """The mode the engine runs in: Q' = fp16(q log2(e) / sqrt(d)) arrives, the kernels scale by exactly 1; reference
    softmax(ln 2 Q' K^T) V in float64 from Q'.  Bars as in B1.  The row maximum of query 0 / head 0 is put into the first, a middle
    and the last 32-key sub-tile in turn."""
    _, B, Hh, T, Tk, d, _ = case
    q, k0, v = unit_inputs(case, seeds=(141, 142, 143), spike=None)
    qs = prescale(q, d)
    for key in dict.fromkeys(spike_keys(Tk)):
        k = k0.clone()
        k[:, key, :d] = q[:, 0, :d] * 4.0
        ref, s = reference(qs, k, v, B, Hh, d, 1.0)
        assert int(s[0, 0, 0].argmax()) == key
        out, region, keep = launch(lib, 'compact', qs, k, v, case, prescaled=1)
        what = f'attention pre-scaled Q {case_id(case)} spike@{key}'
        assert relerr(out.t[region].float().cpu(), ref) < TOL, what
        close(what, out.t[region], ref, local=2 * TOL)


# -------------------------------------------------------------------------------------------------------- B3 logit regimes
# Constants chosen so that the policy emulation alone stays inside the family bar at every head width (checked on the CPU); all
# gains are in operand units, all rates in log2 units of the final logit, i.e. after the factor log2(e) / sqrt(d).
CLIMB_Q = 4.0            # every query's component along the shared direction
CLIMB_NOISE = 0.5        # gain of the random parts of q and k in climb / fall: the trend, not the noise, moves the maximum
LATE_LEAD = 24.0         # log2 units by which the late key leads an average key
DOMINANT_GAIN = 12.0     # q_i = DOMINANT_GAIN * (its key, normalised to |k| = sqrt(d)): own logit 12 log2(e) sqrt(d) log2 units
REGIMES = ('large', 'all_negative', 'flat', 'mixed_rows', 'climb_7.5', 'fall_7.5', 'climb_9', 'fall_9', 'late_maximum',
           'dominant_key')
FAMILY = ('large', 'all_negative', 'flat')      # the three of test_attention_logit_ranges_d40


def _shared_direction(d):
    return torch.full((d,), d ** -0.5)


def _orthogonal_to(x, u, Hh, d):
    """remove the component along u from every head slice of x [B, n, H d]"""
    xh = x.view(x.shape[0], x.shape[1], Hh, d)
    return (xh - (xh * u).sum(-1, keepdim=True) * u).reshape(x.shape)


def regime_inputs(name, case):
    """(q, k, v) fp16-rounded float tensors [B, T, C], [B, Tk, C], [B, Tk, C]; seeded, built on the host"""
    _, B, Hh, T, Tk, d, _ = case
    Cc = Hh * d
    q, k, v = rnd((B, T, Cc), 71), rnd((B, Tk, Cc), 72), h16(rnd((B, Tk, Cc), 73))
    u = _shared_direction(d)
    unit = math.sqrt(d) / LOG2E                  # q.k that makes one log2 unit of logit
    if name == 'large':
        q, k = q * 6.0, k * 6.0
    elif name == 'all_negative':
        q, k = (q * 3.0).abs() + 2.0, -((k * 3.0).abs() + 2.0)        # every q.k strongly negative
    elif name == 'flat':
        q, k = q * 0.05, k * 0.05
    elif name == 'mixed_rows':
        # the rescale branch is wave-uniform: flat and large rows alternate inside every 32-query wave
        gain = torch.where(torch.arange(T) % 2 == 0, 0.05, 6.0).view(1, T, 1)
        q, k = q * gain, k * 6.0
    elif name.startswith(('climb', 'fall')):
        # the logits of every row rise (fall) by `rate` log2 units per 64 keys along one shared direction: at 7.5 the deferred
        # maximum (raised when a tile outgrows it by more than 2^8) lags by tiles, at 9 it is raised on every tile
        rate = float(name.split('_')[1])
        j = torch.arange(Tk, dtype=torch.float32)
        if name.startswith('fall'):
            j = (Tk - 1) - j
        cj = (rate * j / 64.0) * unit / CLIMB_Q
        q = _orthogonal_to(q * CLIMB_NOISE, u, Hh, d) + (CLIMB_Q * u).repeat(Hh)
        k = k * CLIMB_NOISE + cj.view(1, Tk, 1) * u.repeat(Hh)
    elif name == 'late_maximum':
        # the row maximum of EVERY query is the last key: in the last, partial key tile (its only key where Tk % 64 == 1)
        q = _orthogonal_to(q, u, Hh, d) + (CLIMB_Q * u).repeat(Hh)
        k[:, Tk - 1] += (LATE_LEAD * unit / CLIMB_Q) * u.repeat(Hh)
    elif name == 'dominant_key':
        # one-hot softmax: each query row copies one key (position drawn per row, batch and head), scaled
        kh = k.view(B, Tk, Hh, d)
        kh = kh / kh.norm(dim=-1, keepdim=True) * math.sqrt(d)
        pos = torch.randint(0, Tk, (B, T, Hh), generator=torch.Generator().manual_seed(74))
        q = DOMINANT_GAIN * torch.gather(kh, 1, pos.unsqueeze(-1).expand(B, T, Hh, d))
        q, k = q.reshape(B, T, Cc), kh.reshape(B, Tk, Cc)
    else:
        raise KeyError(name)
    return h16(q), h16(k), v


def check_regime_shape(name, case, s):
    """the property a regime is named after, asserted on the float64 logits (log2 units) [B, H, T, Tk]"""
    Tk = case[4]
    if name == 'late_maximum':
        assert bool((s.argmax(-1) == Tk - 1).all()), 'late maximum: some row has its maximum elsewhere'
    if name == 'dominant_key' and Tk > 1:
        top = s.topk(2, -1).values
        assert float((top[..., 0] - top[..., 1]).min()) >= 30.0, 'dominant key: a lead below 30 log2 units'
    if name.startswith('climb') and Tk >= 128:
        assert bool((s.argmax(-1) >= Tk - 64).all())
    if name.startswith('fall') and Tk >= 128:
        assert bool((s.argmax(-1) < 64).all())


def record(line):
    """measured errors: printed, and appended to the file FGDM_ATTN_PARITY_LOG names when it is set
    (profiles/attention_call_parity_errors.txt is a copy of one such run)"""
    print(line)
    path = os.environ.get('FGDM_ATTN_PARITY_LOG')
    if path:
        with open(path, 'a') as f:
            f.write(line + '\n')


def regime_bars(name, case, emu_err, emu_blk):
    """large / all-negative / flat on the kernel they were measured on (the two-strand d = 40 kernel of
    test_attention_logit_ranges_d40) keep that test's bars: normwise 2 TOL, blockwise 4 TOL.  Everywhere else nobody has a number:
    the bar is the larger of that family bar and 1.5 x the error of the policy emulation against the same float64 reference
    (1.5: the deferred maximum leaves P up to 2^8 above 1, which rounds differently from the emulation's exact maximum, while a
    wrong rescale or a dropped tile moves the result by whole units)."""
    if name in FAMILY and case[0] == AD.TWO_STRAND_32 and case[5] == 40:
        return 2 * TOL, 4 * TOL
    return max(2 * TOL, 1.5 * emu_err), max(4 * TOL, 1.5 * emu_blk)


@pytest.mark.parametrize('prescaled', (0, 1), ids=('scaled_in_kernel', 'prescaled_q'))
@pytest.mark.parametrize('name', REGIMES)
@pytest.mark.parametrize('case', REGIME_CASES, ids=case_id)
def test_attention_logit_regimes(lib, case, name, prescaled):
    _, B, Hh, T, Tk, d, _ = case
    q, k, v = regime_inputs(name, case)
    if prescaled:
        q = prescale(q, d)
    ref, s = reference(q, k, v, B, Hh, d, 1.0 if prescaled else LOG2E / math.sqrt(d))
    check_regime_shape(name, case, s)
    emu = emulate(q, k, v, B, Hh, d, prescaled)
    emu_err, emu_blk = relerr(emu, ref), tile_err(emu, ref)
    bar, bar_blk = regime_bars(name, case, emu_err, emu_blk)
    out, region, keep = launch(lib, 'compact', q, k, v, case, prescaled=prescaled)
    got = out.t[region]
    err, blk = relerr(got.float().cpu(), ref), tile_err(got, ref)
    mode = 'prescaled' if prescaled else 'scaled'
    record(f'{AD.KERNEL_NAMES[want_kernel(case)]} d{d} B{B} H{Hh} T{T} Tk{Tk} {name} {mode}: rel_err={err:.3e} tile_err={blk:.3e} '
           f'emulation rel_err={emu_err:.3e} tile_err={emu_blk:.3e} bars {bar:.1e} / {bar_blk:.1e} '
           f'ratio {max(err / bar, blk / bar_blk):.3f} |logit|max {float(s.abs().max()):.0f}')
    if bar > 2 * TOL or bar_blk > 4 * TOL:
        print(f'  the emulation term is the operative bar here: {bar:.3e} / {bar_blk:.3e}')
    assert err < bar, (case_id(case), name, mode, err, bar)
    assert blk < bar_blk, (case_id(case), name, mode, 'tile_err', blk, bar_blk)


def test_two_strand_16_wide_kernel_under_its_knob():
    """attn_dq_kernel<40> is reached only under FGDM_ATTN_DQ=1, read once per process: a fresh interpreter runs the d = 40
    two-strand cases of this module, where want_kernel() then demands the 16-wide kernel."""
    env = dict(os.environ, FGDM_ATTN_DQ='1')
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-q', '-x', '-m', 'gpu', '-k',
                        'two_strand_32_d40 and not under_its_knob'], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:]
    assert ' passed' in r.stdout and 'skipped' not in r.stdout and 'deselected' in r.stdout, r.stdout[-1000:]


# ----------------------------------------------------------------------------------------------------- B4 small_attn_kernel
SMALL_T = (1, 2, 63, 64, 65, 77, 127, 128)
SMALL_D = 64


def small_inputs(B, heads, T, gain, seed=91):
    return h16(rnd((B * T, 3 * heads * SMALL_D), seed) * gain)


def small_reference(qkv, B, heads, T, causal):
    """float64 softmax(q k^T d^-1/2, j <= i when causal) v -> [B T, W]"""
    W = heads * SMALL_D
    q, k, v = (heads_of(qkv[:, i * W:(i + 1) * W].reshape(B, T, W), B, heads, SMALL_D).double() for i in range(3))
    s = torch.matmul(q, k.transpose(-1, -2)) * SMALL_D ** -0.5
    if causal:
        s = s.masked_fill(torch.ones(T, T, dtype=torch.bool).triu(1), float('-inf'))
    return rows_of(torch.matmul(s.softmax(-1), v), B, heads, SMALL_D)


def small_launch(lib, qkv, B, heads, T, causal, gaps, d=SMALL_D):
    """gaps False: the engine's call (ld = 3 W, ldo = W); True: ld = 3 W + 8, ldo = W + 8, input gaps NaN"""
    W = heads * SMALL_D
    ld, ldo = (3 * W + 8, W + 8) if gaps else (3 * W, W)
    buf = strided_in(qkv.half(), ld)
    out = guarded_out((B * max(T, 1), ldo), torch.half)
    rc = lib.fgdm_op_small_attention(vp(buf.data_ptr()), ld, W, 2 * W, vp(out.data_ptr()), ldo, B, heads, T, d, causal, _st())
    torch.cuda.synchronize()
    return rc, out, (slice(None), slice(0, W)), (slice(None), slice(W, ldo))


@pytest.mark.parametrize('heads', (12, 1))
@pytest.mark.parametrize('causal', (1, 0))
@pytest.mark.parametrize('T', SMALL_T)
def test_small_attention(lib, T, causal, heads):
    """fp32 probabilities, fp16 output: the plain per-kernel bars TOL / LOCAL_TOL"""
    B = 3
    for gain, regime in ((1.0, 'unit'), (6.0, 'large')):
        qkv = small_inputs(B, heads, T, gain)
        ref = small_reference(qkv, B, heads, T, causal)
        for gaps in (False, True):
            rc, out, region, gap = small_launch(lib, qkv, B, heads, T, causal, gaps)
            assert rc == 0
            out.check(region)
            if gaps:
                out.assert_untouched(gap)
            close(f'small attention T{T} causal{causal} heads{heads} {regime} gaps{int(gaps)}', out.t[region], ref, TOL, LOCAL_TOL)


@pytest.mark.parametrize('T,d', [(0, 64), (129, 64), (77, 32)])
def test_small_attention_rejects_unsupported_shapes(lib, T, d):
    """FGDM_ERR_ARG before any launch: nothing is written"""
    B, heads = 2, 2
    qkv = small_inputs(B, heads, max(T, 1), 1.0)
    rc, out, region, gap = small_launch(lib, qkv, B, heads, T, 1, False, d=d)
    assert rc == -1
    out.check_guards()
    out.assert_untouched((slice(None), slice(None)))


def test_small_attention_causality_is_bitwise(lib):
    """Row i of a causal call depends on rows <= i only, and its arithmetic does not depend on T: masked scores are -inf, their
    probabilities exactly 0, each lane's share of a row and the shuffle tree are the same for every T, and the PV sum stops at
    j = i.  So the first n rows of the T = 77 output equal the output of a T = n call on the first n rows, bit for bit."""
    B, heads, T = 3, 12, 77
    W = heads * SMALL_D
    qkv = small_inputs(B, heads, T, 1.0)
    rc, full, region, _ = small_launch(lib, qkv, B, heads, T, 1, False)
    assert rc == 0
    full = full.check(region)[region].view(B, T, W)
    for n in (1, 2, 33, 64, 65, 76):
        part_in = qkv.view(B, T, 3 * W)[:, :n].reshape(B * n, 3 * W)
        rc, part, region, _ = small_launch(lib, part_in, B, heads, n, 1, False)
        assert rc == 0
        assert torch.equal(part.check(region)[region].view(B, n, W), full[:, :n]), n
