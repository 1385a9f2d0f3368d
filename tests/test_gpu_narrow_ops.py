"""Per-kernel parity for the kernels and call patterns no other fgdm_op_* entry reaches (they were only ever judged through a whole
network, at 1.09 x floor of a whole tensor):

  B1  convolutions whose Cin is not a multiple of 64 -- the first convolution of every network: Engine::conv3's im2col route
      (conv3_kmap packing, k_im2col<4> / k_im2col<8>, a LINEAR GEMM over K = roundup64(9 cin_pad)) through fgdm_op_conv2d.
      Reference: F.conv2d in float64 on the fp16-rounded input and weights.  Bars: the project's own (normwise TOL = 1e-3,
      blockwise LOCAL_TOL on 32 x 32 blocks) plus the BORDER pixels of every image (first / last output row and column as one
      [rows, Cout] matrix) normwise under LOCAL_TOL whenever they number at least 1024 elements.
      Pad-channel contract (include/fgdm.h): the channels [Cin, cin_pad) of the input must be finite; their weight columns are
      exactly zero, so a finite non-zero value there changes no bit of the result -- asserted here.
  B2  the first-stage AttnBlock core (Engine::vattn_fwd's per-image loop, vattn_core) through fgdm_op_vae_attention, and
      k_softmax_rows on its own.  Reference: softmax(q k^T C^-1/2) v in float64 on the fp16-rounded operands, per image.  Bars as
      for the flash kernels (P is rounded to fp16 before the PV product): normwise TOL, blockwise 2 TOL.
  B3  the layout / elementwise kernels of elementwise.hip: exact or derived answers, no measured tolerance.

Every output sits in a guarded, poisoned buffer, every activation input between NaN guards (tests/guarded.py).  The measured
errors are printed and appended to the file FGDM_NARROW_PARITY_LOG names when it is set (profiles/narrow_ops_parity_errors.txt is
a copy of one such run)."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from common import relerr, report
from guarded import LOCAL_TOL, guarded_in, guarded_out, tile_err
from test_gpu_ops import TOL, _p, _st, close, din, h16, rnd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def lib():
    from fgdm_amd import _lib
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return _lib.load()


def record(line):
    print(line)
    path = os.environ.get('FGDM_NARROW_PARITY_LOG')
    if path:
        with open(path, 'a') as f:
            f.write(line + '\n')


def ulp16(ref):
    """the fp16 unit in the last place at the magnitude of `ref` (float64); below the smallest normal: the subnormal spacing"""
    e = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -14)))
    return torch.pow(2.0, e - 10)


# ===================================================================================================== B1 narrow convolutions
def cin_pad(cin):
    """the rule of the engine's weight packing (conv3_kmap, engine.hip)"""
    g = 8 if cin % 8 == 0 else 4
    return (cin + g - 1) // g * g


def _n(B, H, W, Cin, Cout, stride=1, act=0, extra=False, tag=''):
    return (B, H, W, Cin, Cout, stride, act, extra, tag)


NARROW_CASES = [
    # UNet / ControlNet conv_in and the adapter input (4 -> 320)
    _n(3, 8, 8, 4, 320, tag='conv_in 4->320 8x8'),
    _n(1, 64, 64, 4, 320, tag='conv_in 4->320 64x64'),
    _n(1, 96, 96, 4, 320, extra=True, tag='conv_in 4->320 96x96 rowvec+resid+scale'),
    # ControlNet.input_hint_block (cldm.py:655-671): every layer at a small size (B = 3) ...
    _n(3, 16, 24, 3, 16, act=1, tag='hint 3->16 16x24 silu'),
    _n(3, 16, 24, 16, 16, act=1, tag='hint 16->16 16x24 silu'),
    _n(3, 16, 24, 16, 32, 2, 1, tag='hint 16->32 s2 16x24 silu'),
    _n(3, 16, 24, 32, 32, act=1, tag='hint 32->32 16x24 silu'),
    _n(3, 16, 24, 32, 96, 2, 1, tag='hint 32->96 s2 16x24 silu'),
    _n(3, 16, 24, 96, 96, act=1, tag='hint 96->96 16x24 silu'),
    _n(3, 16, 24, 96, 256, 2, 1, tag='hint 96->256 s2 16x24 silu'),
    # ... and at its real size (B = 1): 262144 rows at 512 x 512, where k_im2col's grid-stride loop wraps (granules > 2^20)
    _n(1, 512, 512, 3, 16, act=1, tag='hint 3->16 512x512 silu'),
    _n(1, 512, 512, 16, 16, act=1, tag='hint 16->16 512x512 silu'),
    _n(1, 512, 512, 16, 32, 2, 1, tag='hint 16->32 s2 512x512 silu'),
    _n(1, 256, 256, 32, 32, act=1, tag='hint 32->32 256x256 silu'),
    _n(1, 256, 256, 32, 96, 2, 1, tag='hint 32->96 s2 256x256 silu'),
    _n(1, 128, 128, 96, 96, act=1, tag='hint 96->96 128x128 silu'),
    _n(1, 128, 128, 96, 256, 2, 1, tag='hint 96->256 s2 128x128 silu'),
    # first-stage conv_in: decoder 4 -> 512, encoder 3 -> 128
    _n(3, 8, 8, 4, 512, tag='vae decoder conv_in 4->512 8x8'),
    _n(1, 64, 64, 4, 512, tag='vae decoder conv_in 4->512 64x64'),
    _n(3, 8, 8, 3, 128, tag='vae encoder conv_in 3->128 8x8'),
    _n(1, 512, 512, 3, 128, tag='vae encoder conv_in 3->128 512x512'),
    # odd and non-square sizes on both strides: every border combination, stride-2 output sizes (H - 1) / 2 + 1
    _n(2, 7, 5, 4, 320, 1, tag='7x5 s1 4->320'),
    _n(2, 7, 5, 4, 320, 2, tag='7x5 s2 4->320'),
    _n(2, 7, 5, 16, 32, 2, tag='7x5 s2 16->32'),
    _n(3, 1, 1, 3, 16, 1, tag='1x1 s1 3->16'),
    _n(3, 1, 1, 96, 256, 2, tag='1x1 s2 96->256'),
    _n(2, 1, 9, 4, 320, 1, tag='1x9 s1 4->320'),
    _n(2, 1, 9, 32, 96, 2, tag='1x9 s2 32->96'),
    _n(2, 17, 3, 3, 16, 1, tag='17x3 s1 3->16'),
    _n(2, 17, 3, 96, 96, 2, tag='17x3 s2 96->96'),
    # M one short of / one past a 128-row tile
    _n(1, 127, 1, 4, 320, tag='M=127 4->320'),
    _n(1, 3, 43, 16, 32, tag='M=129 16->32'),
    _n(1, 1, 129, 3, 128, tag='M=129 3->128'),
    # epilogue kinds on this route
    _n(2, 16, 16, 4, 320, act=0, tag='epilogue bias only'),
    _n(2, 16, 16, 32, 96, act=0, extra=True, tag='epilogue rowvec+resid+scale'),
    _n(2, 16, 16, 16, 16, act=1, extra=True, tag='epilogue silu rowvec+resid+scale'),
    _n(2, 16, 16, 4, 320, act=2, tag='epilogue relu (adapter block1)'),
]
FORCE_CASES = [NARROW_CASES[3], NARROW_CASES[8], NARROW_CASES[1]]       # N = 16 (K = 64), N = 96 (K = 896), N = 320 (K = 64)


@functools.lru_cache(maxsize=2)
def narrow_problem(case):
    """(x NCHW fp16-rounded, w, bias, rowvec, resid, scale, ref float64 NCHW): seeded, built on the host, reference once per case"""
    B, H, W, Cin, Cout, stride, act, extra, tag = case
    x = h16(rnd((B, Cin, H, W), 1))
    w = h16(rnd((Cout, Cin, 3, 3), 2, 1.0 / np.sqrt(Cin * 9)))
    bias = rnd((Cout,), 3, 0.1)
    ref = F.conv2d(x.double(), w.double(), bias.double(), stride=stride, padding=1)
    Ho, Wo = ref.shape[2:]
    assert (Ho, Wo) == ((H - 1) // stride + 1, (W - 1) // stride + 1)
    rowvec = rnd((B, Cout), 4, 0.5) if extra else None
    resid = h16(rnd((B, Cout, Ho, Wo), 5)) if extra else None
    if rowvec is not None:
        ref = ref + rowvec.double()[:, :, None, None]
    if act == 1:
        ref = F.silu(ref)
    elif act == 2:
        ref = F.relu(ref)
    scale = 0.75 if extra else 1.0
    ref = ref * scale
    if resid is not None:
        ref = ref + resid.double()
    return x, w, bias, rowvec, resid, scale, ref


def padded_nhwc(x, cp, pad_value=0.0):
    """NCHW fp32 cpu -> NHWC fp16 with cp channels on the device, between NaN guards; pad channels = pad_value"""
    B, Cin, H, W = x.shape
    xp = torch.full((B, H, W, cp), pad_value, dtype=torch.half)
    xp[..., :Cin] = x.permute(0, 2, 3, 1).half()
    return guarded_in(xp)


def run_narrow(lib, case, pad_value=0.0):
    B, H, W, Cin, Cout, stride, act, extra, tag = case
    x, w, bias, rowvec, resid, scale, ref = narrow_problem(case)
    Ho, Wo = ref.shape[2:]
    x0 = padded_nhwc(x, cin_pad(Cin), pad_value)
    out = guarded_out((B * Ho * Wo, Cout), torch.half)
    # keep every device tensor referenced until the call returns (a temporary's block would be recycled)
    wd, bd = w.cuda(), bias.cuda()
    rvd = din(rowvec) if rowvec is not None else None
    rsd = din(resid.permute(0, 2, 3, 1).half()) if resid is not None else None
    rc = lib.fgdm_op_conv2d(_p(x0), Cin, None, 0, _p(wd), _p(bd), _p(rvd), _p(rsd), B, H, W, Cout, 3, stride, 0, act, scale,
                            _p(out.t), _st())
    assert rc == 0, (tag, rc)
    torch.cuda.synchronize()
    return out.check(), ref


def border_rows(t, B, Ho, Wo):
    """[B Ho Wo, C] -> the rows of the first / last output row and column of every image"""
    m = torch.zeros(Ho, Wo, dtype=torch.bool)
    m[0, :] = m[-1, :] = m[:, 0] = m[:, -1] = True
    return t.view(B, Ho * Wo, -1)[:, m.view(-1).to(t.device)].reshape(-1, t.shape[-1])


def check_narrow(what, got, ref):
    B, Cout, Ho, Wo = ref.shape
    rows = ref.permute(0, 2, 3, 1).reshape(-1, Cout).cuda()
    e, te = close(what, got, rows)
    gb, rb = border_rows(got, B, Ho, Wo), border_rows(rows, B, Ho, Wo)
    be = relerr(gb, rb)
    held = gb.numel() >= 1024
    record(f'{what}: rel_err={e:.3e} tile_err={te:.3e} border_err={be:.3e} ({gb.numel()} border elements'
           f'{"" if held else ", below 1024: recorded only"}) bars {TOL:.1e} / {LOCAL_TOL:.1e} / {LOCAL_TOL:.1e}')
    if held:
        assert be < LOCAL_TOL, (what, 'border', be)


@pytest.mark.parametrize('case', NARROW_CASES, ids=[c[-1] for c in NARROW_CASES])
def test_narrow_conv(lib, case):
    got, ref = run_narrow(lib, case)
    check_narrow(f'narrow conv {case[-1]}', got, ref)


@pytest.mark.parametrize('case', [NARROW_CASES[3], NARROW_CASES[28], NARROW_CASES[20]], ids=lambda c: c[-1])
def test_narrow_conv_pad_channel_does_not_matter(lib, case):
    """Cin = 3: the fourth input channel non-zero (finite) and the weight unchanged gives the same bits: the pad column of the
    packed weight is exactly zero (the contract include/fgdm.h states for the pad channels)."""
    assert case[3] == 3 and cin_pad(3) == 4
    zero, _ = run_narrow(lib, case, 0.0)
    zero = zero.clone()
    other, _ = run_narrow(lib, case, 1.75)
    assert torch.equal(zero.view(torch.int16), other.view(torch.int16)), case[-1]


@pytest.mark.parametrize('cfg', (0, 1), ids=('auto tile', '2-stage 128x128'))
@pytest.mark.parametrize('case', FORCE_CASES, ids=lambda c: c[-1])
def test_narrow_conv_forced_tiles(lib, case, cfg):
    """whatever tile the dispatcher picks for N = 16 / 96 / 320 on a K = 64 ... 896 linear, and the 2-stage 128 x 128 tile"""
    assert lib.fgdm_debug_force_igemm_cfg(cfg) == 0
    try:
        got, ref = run_narrow(lib, case)
    finally:
        lib.fgdm_debug_force_igemm_cfg(0)
    check_narrow(f'narrow conv {case[-1]} force_cfg {cfg}', got, ref)


# ================================================================================================= B2 first-stage attention
K_PAD_ROWS = 128
VATTN_REGIMES = ('unit', 'spike', 'one_key', 'flat', 'all_negative', 'k_pad_large')


def vattn_inputs(regime, B, T, Cc):
    """(q, k, v) fp16-rounded float [B, T, C]; every image different (one seeded draw over the batch)"""
    q, k, v = rnd((B, T, Cc), 71), rnd((B, T, Cc), 72), h16(rnd((B, T, Cc), 73))
    if regime == 'spike':                       # one key spiked against one query, per image at a different place
        for b in range(B):
            k[b, (5 + 17 * b) % T] = q[b, (3 + 7 * b) % T] * 4.0
    elif regime == 'one_key':                   # logits of 300: all probability on one key, drawn per row
        k = k / k.norm(dim=-1, keepdim=True) * math.sqrt(Cc)
        pos = torch.randint(0, T, (B, T), generator=torch.Generator().manual_seed(74))
        q = (300.0 / math.sqrt(Cc)) * torch.gather(k, 1, pos.unsqueeze(-1).expand(B, T, Cc))
    elif regime == 'flat':
        q, k = q * 0.05, k * 0.05
    elif regime == 'all_negative':              # every q.k strongly negative
        q, k = (q * 3.0).abs() + 2.0, -((k * 3.0).abs() + 2.0)
    else:
        assert regime in ('unit', 'k_pad_large')
    return h16(q), h16(k), v


@functools.lru_cache(maxsize=4)
def vattn_problem(regime, B, T, Cc):
    q, k, v = vattn_inputs(regime, B, T, Cc)
    ref = torch.empty(B, T, Cc, dtype=torch.float64)
    smax = 0.0
    for b in range(B):
        s = q[b].double() @ k[b].double().T * Cc ** -0.5
        smax = max(smax, float(s.abs().max()))
        if regime == 'one_key':
            top = s.topk(2, -1).values
            assert float((top[:, 0] - top[:, 1]).min()) > 30.0
        if regime == 'all_negative':
            assert float(s.max()) < -50.0
        ref[b] = torch.softmax(s, -1) @ v[b].double()
    return q, k, v, ref, smax


def run_vattn(lib, q, k, v, pad_value=0.0):
    """q, k, v [B, T, C] -> guarded out [B T, C].  k gets the contract's 128 pad rows (pad_value), NaN guards after them"""
    B, T, Cc = q.shape
    kp = torch.full((B * T + K_PAD_ROWS, Cc), pad_value, dtype=torch.half)
    kp[:B * T] = k.reshape(B * T, Cc).half()
    qd, kd = din(q.reshape(B * T, Cc).half()), guarded_in(kp)
    vtd = din(v.permute(0, 2, 1).half())                   # [B, C, T]; C % 128 == 0 here: NaN guards follow directly
    out = guarded_out((B * T, Cc), torch.half)
    rc = lib.fgdm_op_vae_attention(_p(qd), _p(kd), _p(vtd), _p(out.t), B, T, Cc, _st())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out.check()


def check_vattn(what, got, ref, smax):
    B, T, Cc = ref.shape
    r = ref.reshape(B * T, Cc).cuda()
    e, te = close(what, got, r, local=2 * TOL)
    record(f'{what}: rel_err={e:.3e} tile_err={te:.3e} bars {TOL:.1e} / {2 * TOL:.1e} |logit|max {smax:.0f}')


@pytest.mark.parametrize('T', (64, 256, 1024, 4096))
@pytest.mark.parametrize('Cc', (512, 128))
def test_vae_attention_sizes(lib, Cc, T):
    """B = 3 different images, then each image alone (B = 1): the loop reuses S and P, so image b must not see image b - 1 --
    each image of the batch equals, bit for bit, the same image run alone."""
    B = 3
    q, k, v, ref, smax = vattn_problem('spike', B, T, Cc)
    got = run_vattn(lib, q, k, v)
    check_vattn(f'vae attention C{Cc} T{T} B{B} spike', got, ref, smax)
    for b in range(B):
        alone = run_vattn(lib, q[b:b + 1], k[b:b + 1], v[b:b + 1])
        check_vattn(f'vae attention C{Cc} T{T} B1 image {b} alone', alone, ref[b:b + 1], smax)
        assert torch.equal(alone.view(torch.int16), got[b * T:(b + 1) * T].view(torch.int16)), \
            f'image {b} of the batch differs from the same image run alone (C {Cc}, T {T})'


@pytest.mark.parametrize('regime', VATTN_REGIMES)
@pytest.mark.parametrize('Cc,T', ((512, 1024), (128, 256)))
def test_vae_attention_logit_regimes(lib, Cc, T, regime):
    B = 3
    q, k, v, ref, smax = vattn_problem(regime, B, T, Cc)
    # k_pad_large: the 128 pad rows of k hold large finite values; they must not reach the output
    got = run_vattn(lib, q, k, v, pad_value=30000.0 if regime == 'k_pad_large' else 0.0)
    check_vattn(f'vae attention C{Cc} T{T} B{B} {regime}', got, ref, smax)
    if regime == 'k_pad_large':
        plain = run_vattn(lib, q, k, v, pad_value=0.0)
        assert torch.equal(plain.view(torch.int16), got.view(torch.int16)), 'the pad rows of k reached the output'


@pytest.mark.parametrize('cfg', (0, 1), ids=('auto tile', '2-stage 128x128'))
@pytest.mark.parametrize('Cc,T', ((512, 64), (512, 256), (128, 1024)))
def test_vae_attention_forced_tiles(lib, Cc, T, cfg):
    """cfg 1 reads whole 128-row weight tiles: at T = 64 the last image's score GEMM reads 64 of k's pad rows.  Wider forced tiles
    would read weight rows beyond what the engine's contract pads; they are not forced here."""
    B = 3
    q, k, v, ref, smax = vattn_problem('unit', B, T, Cc)
    assert lib.fgdm_debug_force_igemm_cfg(cfg) == 0
    try:
        got = run_vattn(lib, q, k, v, pad_value=30000.0)
    finally:
        lib.fgdm_debug_force_igemm_cfg(0)
    check_vattn(f'vae attention C{Cc} T{T} B{B} unit force_cfg {cfg}', got, ref, smax)


SOFTMAX_ROWS = 70


def softmax_logits(cols):
    s = rnd((SOFTMAX_ROWS, cols), 81, 3.0)
    s[1] = rnd((cols,), 82, 30.0)
    s[2, cols // 3] += 1000.0                   # one + large entry: one-hot
    s[3, cols - 1] -= 1000.0                    # one - large entry: exactly zero there
    s[4] = 0.0                                  # constant rows
    s[5] = 7.25
    s[6] = -60000.0                             # a row of all -60000
    s[7, 0] += 500.0                            # the large entry in the first / last column (first / last wave of the block)
    s[8, cols - 1] += 500.0
    return s


@pytest.mark.parametrize('cols', (64, 200, 256, 1000, 4096))
def test_softmax_rows(lib, cols):
    """k_softmax_rows against float64 softmax rounded to fp16: every element within one fp16 ulp (taken at the reference's
    magnitude; where the reference is an fp16 subnormal: within 2^-14 absolute, the smallest normal, so that a flush-to-zero
    conversion is recorded and not failed); row sums within cols * 2^-12 of 1 (fp16 half-ulp per element at most: derived)."""
    s = softmax_logits(cols)
    ref = torch.softmax(s.double(), -1).half().double()
    sd = din(s)
    out = guarded_out((SOFTMAX_ROWS, cols), torch.half)
    assert lib.fgdm_op_softmax_rows(_p(sd), _p(out.t), SOFTMAX_ROWS, cols, _st()) == 0
    torch.cuda.synchronize()
    got = out.check().double().cpu()
    d = (got - ref).abs()
    normal = ref >= 2.0 ** -14
    ulps = float((d[normal] / ulp16(ref[normal])).max())
    sub = float(d[~normal].max()) if bool((~normal).any()) else 0.0
    flushed = int(((got == 0) & (ref > 0) & ~normal).sum())
    sums = float((got.sum(-1) - 1.0).abs().max())
    record(f'softmax_rows cols {cols}: worst deviation {ulps:.2f} fp16 ulp (bound 1); subnormal references: worst {sub:.3e} absolute '
           f'(bound {2.0 ** -14:.3e}), {flushed} of {int((~normal).sum())} returned as zero; worst |row sum - 1| {sums:.3e} '
           f'(bound {cols * 2.0 ** -12:.3e})')
    assert ulps <= 1.0, (cols, ulps)
    assert sub <= 2.0 ** -14, (cols, sub)
    assert sums <= cols * 2.0 ** -12, (cols, sums)
    assert float(got[2, cols // 3]) == 1.0 and float(got[3, cols - 1]) == 0.0
    assert float(got[7, 0]) == 1.0 and float(got[8, cols - 1]) == 1.0


# ============================================================================================ B3 layout / elementwise kernels
LAYOUT_CASES = [(B, Cc, Cp, HW) for (Cc, Cp) in ((3, 4), (4, 4), (320, 320)) for HW in (1, 63, 4096, 512 * 512) for B in (1, 3)
                if Cc < 320 or HW <= 4096]


@pytest.mark.parametrize('B,Cc,Cp,HW', LAYOUT_CASES)
def test_layout_kernels(lib, B, Cc, Cp, HW):
    """nchw_to_nhwc: bit-equal to x.permute(...).half(), pad channels exactly +0; nhwc_to_nchw: bit-equal to .float() of the
    permuted input; the round trip of fp16-representable data is the identity.  (3, *, 512 x 512) and (3, 320, 4096) exceed 2^20
    elements: the grid-stride loop wraps."""
    x = rnd((B, Cc, HW), 91)
    xd = din(x)
    out = guarded_out((B, HW, Cp), torch.half)
    assert lib.fgdm_op_nchw_to_nhwc(_p(xd), _p(out.t), B, Cc, HW, Cp, _st()) == 0
    torch.cuda.synchronize()
    got = out.check().cpu()
    want = torch.zeros(B, HW, Cp, dtype=torch.half)
    want[..., :Cc] = x.permute(0, 2, 1).half()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), 'nchw_to_nhwc (pad channels must be +0)'
    # back: the compact [B, HW, C] fp16 tensor -> fp32 NCHW
    y = want[..., :Cc].contiguous()
    yd = din(y)
    back = guarded_out((B, Cc, HW), torch.float32)
    assert lib.fgdm_op_nhwc_to_nchw(_p(yd), _p(back.t), B, Cc, HW, _st()) == 0
    torch.cuda.synchronize()
    gb = back.check().cpu()
    assert torch.equal(gb.view(torch.int32), y.permute(0, 2, 1).float().contiguous().view(torch.int32)), 'nhwc_to_nchw'
    assert torch.equal(gb, x.half().float()), 'round trip of fp16-representable data'
    record(f'layout B{B} C{Cc}->{Cp} HW{HW} ({B * HW * Cp} elements): nchw_to_nhwc, nhwc_to_nchw and the round trip bit-equal')


@pytest.mark.parametrize('Cc', (8, 320))
@pytest.mark.parametrize('H,W', ((2, 2), (64, 96), (6, 10)))
def test_avgpool2(lib, Cc, H, W):
    """every element within one fp16 ulp of F.avg_pool2d in float64 (the sum of four fp16 values in fp32 is correct to far below
    an fp16 ulp, so the result is the correctly rounded value or its neighbour); no share of elements exempt"""
    B = 3
    x = h16(rnd((B, Cc, H, W), 92, 2.0))
    ref = F.avg_pool2d(x.double(), 2).permute(0, 2, 3, 1).contiguous()
    xd = din(x.permute(0, 2, 3, 1).half())
    out = guarded_out((B, H // 2, W // 2, Cc), torch.half)
    assert lib.fgdm_op_avgpool2(_p(xd), _p(out.t), B, H, W, Cc, _st()) == 0
    torch.cuda.synchronize()
    got = out.check().double().cpu()
    worst = float(((got - ref).abs() / ulp16(ref)).max())
    exact = float((got == ref.half().double()).double().mean())
    record(f'avgpool2 B{B} {H}x{W} C{Cc}: worst deviation {worst:.3f} fp16 ulp (bound 1); {100 * exact:.2f} % correctly rounded')
    assert worst <= 1.0, worst


@pytest.mark.parametrize('Cc', (320, 1280))
@pytest.mark.parametrize('Tk', (77, 154, 231, 1, 64))
def test_transpose_pad(lib, Tk, Cc):
    B, Tkpad = 2, (Tk + 63) // 64 * 64
    v = rnd((B, Tk, Cc), 93).half()
    vd = din(v)
    out = guarded_out((B, Cc, Tkpad), torch.half)
    assert lib.fgdm_op_transpose_pad(_p(vd), _p(out.t), B, Tk, Cc, Tkpad, _st()) == 0
    torch.cuda.synchronize()
    got = out.check().cpu()
    assert torch.equal(got[:, :, :Tk].contiguous().view(torch.int16), v.permute(0, 2, 1).contiguous().view(torch.int16))
    assert bool((got[:, :, Tk:].contiguous().view(torch.int16) == 0).all()), 'pad columns must be exactly +0'
    record(f'transpose_pad B{B} Tk{Tk}->{Tkpad} C{Cc}: bit-equal, pad columns +0, guards intact')


@pytest.mark.parametrize('n', (8, 2 ** 20 + 8, 8 * (2 ** 20 + 3)))
def test_add_f16(lib, n):
    """the exact fp32 sum of two fp16 values rounds correctly: bit-equal to (a.float() + b.float()).half(), hence within one
    fp16 ulp (in fact half) of the float64 sum.  n / 8 > 2^20 vectors: the grid-stride loop wraps."""
    a, b = rnd((n,), 94, 3.0).half(), rnd((n,), 95, 3.0).half()
    ad, bd = din(a), din(b)
    out = guarded_out((n,), torch.half)
    assert lib.fgdm_op_add_f16(_p(ad), _p(bd), _p(out.t), n, _st()) == 0
    torch.cuda.synchronize()
    got = out.check().cpu()
    assert torch.equal(got.view(torch.int16), (a.float() + b.float()).half().view(torch.int16))
    ref = a.double() + b.double()
    worst = float(((got.double() - ref).abs() / ulp16(ref)).max())
    record(f'add_f16 n {n}: bit-equal to the fp32 sum rounded once; worst deviation from the float64 sum {worst:.3f} fp16 ulp (bound 1)')
    assert worst <= 1.0


T_INT = (0, 1, 37, 500, 999)
T_FRAC = (949.05, 0.5, 999.99)


def timestep_reference(t32, dim):
    """timestep_embedding (ldm/modules/diffusionmodules/util.py:160-180, as oracle/nn.py restates it) in float64 on the fp32
    value of t -> (embedding [B, dim], per-element bound)"""
    half = dim // 2
    kk = torch.arange(half, dtype=torch.float64)
    freqs = torch.exp(-math.log(10000.0) * kk / half)
    args = t32.double()[:, None] * freqs[None]
    emb = torch.cat([torch.cos(args), torch.sin(args)], dim=-1)
    xk = 9.2103 * kk / half
    bound = 2.0 ** -12 + args.abs() * (3 * xk + 6)[None] * 2.0 ** -24 + 2.0 ** -22
    return emb, torch.cat([bound, bound], dim=-1)


@pytest.mark.parametrize('dim', (320, 64))
def test_timestep_embed(lib, dim):
    """Per element |got - ref| <= 2^-12 + |arg| (3 x_k + 6) 2^-24 + 2^-22 with x_k = 9.2103 k / half, arg = t f_k: the fp16 store's
    half ulp for |v| <= 1; three relative roundings of 2^-24 on the exponent x_k (each an equal relative error of f_k), expf within
    2 ulp, the product t f_k and the float value of t one rounding each; cosf / sinf within 2 ulp absolute.  At most about 6e-4
    (k = 0, t = 999), fixed in advance."""
    B, rows_pad = len(T_INT), len(T_INT) + 11
    ti = torch.tensor(T_INT, dtype=torch.int64)
    tid, tfd = din(ti), din(ti.float())
    oi, of = guarded_out((rows_pad, dim), torch.half), guarded_out((rows_pad, dim), torch.half)
    assert lib.fgdm_op_timestep_embed(_p(tid), None, _p(oi.t), B, dim, rows_pad, _st()) == 0
    assert lib.fgdm_op_timestep_embed(None, _p(tfd), _p(of.t), B, dim, rows_pad, _st()) == 0
    torch.cuda.synchronize()
    gi, gf = oi.check().cpu(), of.check().cpu()
    assert torch.equal(gi.view(torch.int16), gf.view(torch.int16)), 'integer t and the same t as float must be bit-equal'
    assert bool((gi[B:].view(torch.int16) == 0).all()), 'rows >= B must be exactly zero'
    tf = torch.tensor(T_FRAC, dtype=torch.float32)
    tfd2 = din(tf)
    o2 = guarded_out((len(T_FRAC), dim), torch.half)           # rows_pad == B
    assert lib.fgdm_op_timestep_embed(None, _p(tfd2), _p(o2.t), len(T_FRAC), dim, len(T_FRAC), _st()) == 0
    torch.cuda.synchronize()
    g2 = o2.check().cpu()
    for name, got, t32 in (('integer t', gi[:B], ti.float()), ('fractional t', g2, tf)):
        ref, bound = timestep_reference(t32, dim)
        d = (got.double() - ref).abs()
        ratio = d / bound
        i = int(ratio.argmax())
        record(f'timestep_embed dim {dim} {name}: worst |got - ref| {float(d.max()):.3e}; worst deviation / bound {float(ratio.max()):.3f} '
               f'(t {float(t32[i // dim])}, column {i % dim}: {float(d.view(-1)[i]):.3e} against {float(bound.view(-1)[i]):.3e}); '
               f'largest bound {float(bound.max()):.3e}')
        assert bool((d <= bound).all()), (name, dim, float(ratio.max()))
        assert relerr(got, ref) < TOL
