"""Per-kernel parity: every HIP kernel, called through the C ABI, against the CPU oracle's arithmetic
(torch fp32 functional on the SAME fp16-rounded inputs and weights).

Tolerance: normwise relative error <= 1e-3 (the north_star's "1e-3 relative fp16 tolerance"); outputs are
stored in fp16 (unit roundoff 4.9e-4), accumulation is fp32.  Next to it, the blockwise error (tests/guarded.py tile_err) stays
under LOCAL_TOL = 2e-3 over 32 x 32 (row, column) blocks: a ragged last tile or one wrong block that the normwise error averages
away fails there.

Every output is written into a guarded buffer (tests/guarded.py): payload poisoned with a NaN bit pattern no kernel produces,
between seeded guard bytes -- an element never written, a store past either end, or a non-finite value fails the case.  Every
activation input sits between NaN guards, so a read past its end that reaches a result shows up as well."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from attention_dispatch import expected_kernel
from common import relerr, report
from guarded import LOCAL_TOL, guarded_in, guarded_out, tile_err

pytestmark = pytest.mark.gpu

TOL = 1e-3


@pytest.fixture(scope='module')
def lib():
    from fgdm_amd import _lib
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return _lib.load()


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def din(t):      # cpu tensor -> device copy between NaN guards
    return guarded_in(t.contiguous())


def nhwc16(x):   # NCHW fp32 cpu -> NHWC fp16 cuda (between NaN guards)
    return din(x.permute(0, 2, 3, 1).half())


def to_rows(x):  # NCHW -> [B H W, C]: the kernels' (row, column) layout, the one tile_err's blocks follow
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])


def close(what, got, ref, tol=TOL, local=LOCAL_TOL, block=(32, 32)):
    """normwise error < tol and blockwise error < local; both recorded"""
    ref = torch.as_tensor(ref).to(got.device)           # both errors in fp64 on the device
    e = relerr(got, ref)
    te = tile_err(got, ref, block)
    report(f'{what} [tile_err {te:.3e}]', e, tol)
    assert e < tol, (what, e)
    assert te < local, (what, 'tile_err', te)
    return e, te


def from_nhwc(y, B, H, W, Cc):
    return y.float().cpu().view(B, H, W, Cc).permute(0, 3, 1, 2)


def h16(x):
    return x.half().float()


CONV_CASES = [
    # B, H, W, C0, C1, Cout, ksize, stride, up, act, extras
    (2, 16, 16, 320, 0, 320, 3, 1, 0, 0, 'bias+rowvec+resid'),
    (2, 8, 8, 640, 320, 320, 3, 1, 0, 1, 'concat+silu'),
    (3, 8, 8, 320, 0, 640, 3, 2, 0, 0, 'stride2, M tail'),
    (2, 8, 8, 640, 0, 640, 3, 1, 1, 0, 'upsample'),
    (1, 1, 1, 1280, 0, 1280, 3, 1, 0, 0, '1x1 spatial'),
    (2, 8, 8, 1280, 640, 1280, 1, 1, 0, 0, 'conv1x1 concat (skip_connection)'),
    (2, 16, 16, 320, 0, 4, 3, 1, 0, 0, 'N=4 (UNet out conv)'),
    (1, 64, 64, 320, 0, 320, 3, 1, 0, 2, 'full-res latent, relu'),
    (2, 7, 5, 64, 0, 96, 3, 2, 0, 0, 'odd sizes'),
    (3, 8, 8, 640, 0, 320, 3, 1, 0, 1, 'split-K (8x8, K=5760) silu + rowvec + resid'),
    (2, 8, 8, 1280, 1280, 1280, 3, 1, 0, 0, 'split-K decoder concat (8x8, K=23040)'),
    (24, 8, 8, 1280, 0, 1280, 3, 1, 0, 0, 'split-K x8 on 256x320 tiles (8x8, K=11520, B=24) rowvec + resid'),
    (25, 8, 8, 1280, 1280, 1280, 3, 1, 0, 0, 'split-K x8 on 256x320 tiles, decoder concat, M tail (B=25)'),
    (2, 16, 16, 1280, 640, 1280, 3, 1, 0, 0, 'split-K x2 (16x16, K=17280) thin tiles rowvec + resid'),
    (25, 16, 16, 1280, 1280, 1280, 3, 1, 0, 1, 'split-K x2 on 256x320 tiles (16x16, K=23040, B=25) silu'),
    (9, 16, 16, 1280, 0, 1280, 3, 1, 0, 0, 'split-K x2 (16x16, K=11520, a layer without a twin) rowvec + resid'),
    # split K with M = 1 or 255 mod 256 (ragged images: rows_per_sample <= 64 splits four / eight ways, 64 < rps <= 256 two ways):
    # the last row tile of every K slice and the reduction pass's tail
    (9, 3, 19, 640, 0, 320, 3, 1, 0, 1, 'split-K x4, M=513 (rps 57) silu + rowvec + resid'),
    (5, 3, 17, 1280, 0, 320, 3, 1, 0, 0, 'split-K x8, M=255 (rps 51)'),
    (3, 9, 19, 1280, 0, 320, 3, 1, 0, 0, 'split-K x2, M=513 (rps 171) rowvec + resid'),
    (1, 15, 17, 1280, 640, 320, 3, 1, 0, 0, 'split-K x2 concat, M=255 (rps 255)'),
]


@pytest.mark.parametrize('case', CONV_CASES, ids=[c[-1] for c in CONV_CASES])
def test_conv(lib, case):
    B, H, W, C0, C1, Cout, ks, stride, up, act, tag = case
    Cin = C0 + C1
    x = h16(rnd((B, Cin, H, W), 1))
    w = h16(rnd((Cout, Cin, ks, ks), 2, 1.0 / np.sqrt(Cin * ks * ks)))
    bias = rnd((Cout,), 3, 0.1)
    ref_in = F.interpolate(x, scale_factor=2, mode='nearest') if up else x
    ref = F.conv2d(ref_in, w, bias, stride=stride, padding=ks // 2)
    Ho, Wo = ref.shape[2:]
    use_extra = 'rowvec' in tag
    rowvec = rnd((B, Cout), 4, 0.5) if use_extra else None
    resid = h16(rnd((B, Cout, Ho, Wo), 5)) if use_extra else None
    if rowvec is not None:
        ref = ref + rowvec[:, :, None, None]
    if act == 1:
        ref = F.silu(ref)
    elif act == 2:
        ref = F.relu(ref)
    scale = 0.75 if use_extra else 1.0
    ref = ref * scale
    if resid is not None:
        ref = ref + resid
    x0 = nhwc16(x[:, :C0])
    x1 = nhwc16(x[:, C0:]) if C1 else None
    out = guarded_out((B * Ho * Wo, Cout), torch.half)
    # keep every device tensor referenced until the call returns (a temporary's block would be recycled)
    wd, bd = w.cuda(), bias.cuda()
    rvd = din(rowvec) if rowvec is not None else None
    rsd = nhwc16(resid) if resid is not None else None
    rc = lib.fgdm_op_conv2d(_p(x0), C0, _p(x1), C1, _p(wd), _p(bd), _p(rvd), _p(rsd),
                            B, H, W, Cout, ks, stride, up, act, scale, _p(out.t), _st())
    assert rc == 0
    torch.cuda.synchronize()
    got = out.check()
    assert relerr(from_nhwc(got, B, Ho, Wo, Cout), ref) < TOL, tag
    close(f'conv {tag}', got, to_rows(ref))


def test_linear_variants(lib):
    M, K, N = 200, 320, 2560
    x = h16(rnd((M, K), 11))
    w = h16(rnd((N, K), 12, 1 / np.sqrt(K)))
    b = rnd((N,), 13, 0.1)
    # GEGLU (ldm/modules/attention.py:37-44): value * gelu(gate), gate = second half of the projection
    y = F.linear(x, w, b)
    a, g = y.chunk(2, dim=-1)
    ref = a * F.gelu(g)
    out = guarded_out((M, N // 2), torch.half)
    xd, wd, bd = din(x.half()), w.cuda(), b.cuda()
    assert lib.fgdm_op_linear(_p(xd), _p(wd), _p(bd), None, M, K, N, 3, 0, 0, 0, _p(out.t), _st()) == 0
    assert relerr(out.check().float().cpu(), ref) < TOL
    close('linear GEGLU', out.t, ref)
    # plain + residual, fp32 output, transposed fp16 output (V^T for attention), ragged rows-per-sample (77)
    N2 = 320
    w2, b2 = w[:N2].contiguous(), b[:N2].contiguous()
    ref = F.linear(x, w2, b2)
    res = h16(rnd((M, N2), 14))
    out = guarded_out((M, N2), torch.half)
    w2d, b2d, resd = w2.cuda(), b2.cuda(), din(res.half())
    assert lib.fgdm_op_linear(_p(xd), _p(w2d), _p(b2d), _p(resd), M, K, N2, 0, 0, 0, 0, _p(out.t), _st()) == 0
    assert relerr(out.check().float().cpu(), ref + res) < TOL
    close('linear + resid', out.t, ref + res)
    out32 = guarded_out((M, N2), torch.float32)
    assert lib.fgdm_op_linear(_p(xd), _p(w2d), _p(b2d), None, M, K, N2, 0, 1, 0, 0, _p(out32.t), _st()) == 0
    assert relerr(out32.check().cpu(), ref) < 2e-5 + 0 * TOL     # fp32 store: only accumulation-order error
    close('linear fp32', out32.t, ref, 2e-5, 2 * 2e-5)      # fp32 store: blockwise 2 x the normwise bar (no fp16 rounding to average)
    for rps, Bt in ((100, 2), (77, 2), (4, 50)):
        Mt = rps * Bt
        ld = (rps + 63) // 64 * 64
        outT = guarded_out((Bt, N2, ld), torch.half)
        xt = din(x[:Mt].half())
        assert lib.fgdm_op_linear(_p(xt), _p(w2d), _p(b2d), None, Mt, K, N2, 0, 3, rps, ld, _p(outT.t), _st()) == 0
        want = ref[:Mt].view(Bt, rps, N2).permute(0, 2, 1)
        check_transposed(outT, rps, ld)
        assert relerr(outT.t[:, :, :rps].float().cpu(), want) < TOL
        close(f'linear V^T rps {rps}', outT.t[:, :, :rps].reshape(-1, rps), want.reshape(-1, rps))


def check_transposed(outT, rps, ld):
    """OUT_F16_T / OUT_F32_NCHW: every (sample, channel, t < rps) written, the pad columns t >= rps NOT: the engine zeroes the
    padded part of V^T once (engine.hip, the attention workspace) and the projections write around it.  Neither kernel's
    transposed epilogue stores to t >= rps (igemm.hip: t = row - b rps with row < M; igemm2.hip's direct path the same, and
    its 16-byte V^T runs only serve the LayerNorm-consumer path with rows_per_sample % 32 == 0, never a pad column)."""
    outT.check((slice(None), slice(None), slice(0, rps)))
    if ld > rps:
        outT.assert_untouched((slice(None), slice(None), slice(rps, None)))


@pytest.mark.parametrize('M,K,N', [(66000, 320, 2560), (16500, 640, 5120)], ids=['L0-like ragged M', 'L1-like ragged M'])
def test_geglu_persistent_kernel(lib, M, K, N):
    """The GEGLU projection (ldm/modules/attention.py:37-64) with more 256 x 256 tiles than CUs runs on the persistent kernel
    (igemm2_geglu_persist_kernel, round 4): 256 workgroups walk the tiles, the next tile's first stages travel behind the current
    epilogue.  Without a folded LayerNorm here (the LayerNorm-folded form is held bitwise against the 2-stage kernel by
    test_layernorm_folded_into_consumer_gemm); M is not a multiple of 256, so the last row tile of every column is ragged, and the
    same call forced onto the one-workgroup-per-tile kernels (phase-locked loop) must give the same bits."""
    x = h16(rnd((M, K), 21))
    w = h16(rnd((N, K), 22, 1 / np.sqrt(K)))
    b = rnd((N,), 23, 0.1)
    a, g = F.linear(x, w, b).chunk(2, dim=-1)
    ref = a * F.gelu(g)
    xd, wd, bd = din(x.half()), w.cuda(), b.cuda()
    out = guarded_out((M, N // 2), torch.half)
    assert lib.fgdm_op_linear(_p(xd), _p(wd), _p(bd), None, M, K, N, 3, 0, 0, 0, _p(out.t), _st()) == 0
    assert relerr(out.check().float().cpu(), ref) < TOL
    close(f'GEGLU persistent M {M}', out.t, ref)     # the ragged last row tile (M % 256 rows) is its own set of blocks
    out2 = guarded_out((M, N // 2), torch.half)
    try:
        lib.fgdm_debug_force_igemm_cfg(5 + 16)          # 256 x 256 tiles, phase-locked K loop: never the persistent kernel
        assert lib.fgdm_op_linear(_p(xd), _p(wd), _p(bd), None, M, K, N, 3, 0, 0, 0, _p(out2.t), _st()) == 0
    finally:
        lib.fgdm_debug_force_igemm_cfg(0)
    assert torch.equal(out.t, out2.check())


GN_CASES = [(2, 64, 320, 0, 1e-5, 1), (2, 64, 1280, 640, 1e-5, 1), (1, 16, 1280, 1280, 1e-5, 1),
            (2, 1, 1280, 0, 1e-6, 0), (3, 4096, 320, 0, 1e-6, 0), (2, 256, 640, 320, 1e-5, 1),
            # 82 KB slices (two-kernel path since round 2), a 41 KB slice (single kernel, second choice), ragged pixel counts,
            # the autoencoder's 128-channel full-resolution level (4 channels per group)
            (2, 1024, 640, 0, 1e-5, 1), (2, 1024, 1280, 0, 1e-5, 1), (1, 256, 1280, 1280, 1e-5, 1),
            (1, 1000, 320, 0, 1e-5, 1), (1, 999, 640, 640, 1e-6, 0), (1, 16384, 128, 0, 1e-6, 1),
            # the register-resident single pass (64x64 / 32x32 levels): every piece count, concat sources inside and across slices,
            # ragged pixel counts, and a width that falls back to two kernels at 64x64 (960)
            (2, 4096, 320, 320, 1e-5, 1), (1, 4096, 640, 320, 1e-5, 1), (2, 1024, 1280, 640, 1e-5, 1), (2, 1024, 640, 320, 1e-6, 0),
            (1, 4090, 320, 0, 1e-5, 1), (2, 1024, 320, 0, 1e-5, 1), (1, 2000, 640, 0, 1e-5, 1)]


@pytest.mark.parametrize('case', GN_CASES, ids=[f'B{c[0]}_HW{c[1]}_C{c[2]}+{c[3]}' for c in GN_CASES])
def test_groupnorm(lib, case):
    B, HW, C0, C1, eps, silu = case
    Cc = C0 + C1
    x = h16(rnd((B, Cc, HW, 1), 21) * 2.0 + 0.7)
    gamma, beta = 1 + 0.2 * rnd((Cc,), 22), 0.1 * rnd((Cc,), 23)
    ref = F.group_norm(x, 32, gamma, beta, eps)
    if silu:
        ref = F.silu(ref)
    out = run_groupnorm(lib, x, C0, gamma, beta, eps, silu)
    assert relerr(from_nhwc(out, B, HW, 1, Cc), ref) < TOL
    close(f'GroupNorm B{B} HW{HW} C{C0}+{C1}', out, to_rows(ref))


def run_groupnorm(lib, x, C0, gamma, beta, eps, silu):
    """x: NCHW [B, C, HW, 1] fp32 (fp16-representable), split at C0 into the two sources of the virtual concat -> guarded,
    checked NHWC output [B HW, C]"""
    B, Cc, HW = x.shape[0], x.shape[1], x.shape[2]
    C1 = Cc - C0
    x0 = nhwc16(x[:, :C0])
    x1 = nhwc16(x[:, C0:]) if C1 else None
    out = guarded_out((B * HW, Cc), torch.half)
    gd, bd = gamma.cuda(), beta.cuda()
    assert lib.fgdm_op_groupnorm(_p(x0), C0, _p(x1), C1, B, HW, _p(gd), _p(bd), eps, silu, _p(out.t), _st()) == 0
    return out.check()


@pytest.mark.parametrize('offset', [8.0, 32.0], ids=lambda o: f'mean{int(o)}std')
@pytest.mark.parametrize('case', GN_CASES, ids=[f'B{c[0]}_HW{c[1]}_C{c[2]}+{c[3]}' for c in GN_CASES])
def test_groupnorm_groups_with_large_mean(lib, case, offset):
    """Every GroupNorm body forms var = E[x^2] - mean^2 from fp32 per-thread sums, which cancels when |mean| >> std.  Each
    (sample, group) shifted by +-`offset` standard deviations (0.5 ... 1.5 x), per-channel jitter of 0.3 std and a few
    outlier channels with six times the spread; every path of GN_CASES (register-resident, single kernel, two kernels, concat
    inside and across slices, ragged HW).  Reference: group_norm in fp64 on the fp16-rounded input."""
    B, HW, C0, C1, eps, silu = case
    Cc = C0 + C1
    x = rnd((B, Cc, HW, 1), 25)
    x[:, ::97] *= 6.0                                                           # outlier channels
    goff = offset * (0.5 + rnd((B, 32), 26).abs()) * torch.sign(rnd((B, 32), 27))
    x = x + goff.repeat_interleave(Cc // 32, dim=1)[:, :, None, None] + 0.3 * rnd((1, Cc, 1, 1), 28)
    x = h16(x)
    gamma, beta = 1 + 0.2 * rnd((Cc,), 22), 0.1 * rnd((Cc,), 23)
    ref = F.group_norm(x.double(), 32, gamma.double(), beta.double(), eps)
    if silu:
        ref = F.silu(ref)
    out = run_groupnorm(lib, x, C0, gamma, beta, eps, silu)
    e, te = close(f'GroupNorm large mean {offset:g} std B{B} HW{HW} C{C0}+{C1}', out, to_rows(ref))
    print(f'GroupNorm, group mean ~{offset:g} x std, B{B} HW{HW} C{C0}+{C1}: rel_err={e:.3e} tile_err={te:.3e}')


def test_groupnorm_is_bitwise_reproducible(lib):
    B, HW, Cc = 2, 1024, 640
    x = nhwc16(rnd((B, Cc, HW, 1), 24))
    gamma, beta = torch.ones(Cc).cuda(), torch.zeros(Cc).cuda()
    outs = []
    for _ in range(3):
        out = guarded_out((B * HW * Cc,), torch.half)
        assert lib.fgdm_op_groupnorm(_p(x), Cc, None, 0, B, HW, _p(gamma), _p(beta), 1e-5, 1, _p(out.t), _st()) == 0
        outs.append(out.check())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


@pytest.mark.parametrize('C_', [320, 640, 1280])
def test_layernorm(lib, C_):
    rows = 333
    x = h16(rnd((rows, C_), 31) * 1.5 + 0.3)
    gamma, beta = 1 + 0.2 * rnd((C_,), 32), 0.1 * rnd((C_,), 33)
    ref = F.layer_norm(x, (C_,), gamma, beta, 1e-5)
    out = guarded_out((rows, C_), torch.half)
    xd, gd, bd = din(x.half()), gamma.cuda(), beta.cuda()
    assert lib.fgdm_op_layernorm(_p(xd), rows, C_, _p(gd), _p(bd), 1e-5, _p(out.t), _st()) == 0
    torch.cuda.synchronize()
    assert relerr(out.check().float().cpu(), ref) < TOL
    close(f'LayerNorm C{C_}', out.t, ref)


ATT_CASES = [(2, 8, 64, 64, 40), (1, 8, 4096, 4096, 40), (2, 8, 1024, 1024, 80), (2, 8, 256, 256, 160),
             (2, 8, 64, 77, 40), (1, 8, 4096, 77, 40), (2, 8, 256, 77, 160), (2, 8, 1, 1, 160), (2, 8, 16, 16, 80),
             (1, 4, 200, 130, 80),
             # the half-tile boundary of the last key tile (second 32-key sub-tile skipped when it starts at or beyond Tk)
             (1, 8, 64, 32, 40), (1, 8, 64, 33, 80), (1, 8, 128, 96, 40), (1, 8, 128, 97, 160),
             # the text-token kernel (64 < Tk <= 96, T >= 128): every head width, ragged T (a wave's last chunk partly / wholly
             # past the end), one and several chunks per wave, the key-count limits
             (2, 8, 1024, 77, 80), (2, 8, 512, 77, 160), (1, 8, 700, 77, 40), (3, 8, 130, 77, 80), (1, 8, 512, 96, 40),
             (1, 8, 640, 65, 80), (2, 4, 256, 77, 160),
             # long self-attention whose T is not a multiple of 256 (or Tk of 64): the eight-wave ping-pong kernel, which the
             # two-strand kernels (round 4) replace only where their shape conditions hold
             (1, 8, 320, 320, 40), (1, 8, 384, 300, 80), (2, 8, 512, 256, 40)]


@pytest.mark.parametrize('case', ATT_CASES, ids=[f'B{c[0]}_H{c[1]}_T{c[2]}_Tk{c[3]}_d{c[4]}' for c in ATT_CASES])
def test_attention(lib, case):
    B, Hh, T, Tk, d = case
    Cc = Hh * d
    q, k, v = h16(rnd((B, T, Cc), 41)), h16(rnd((B, Tk, Cc), 42)), h16(rnd((B, Tk, Cc), 43))
    # spike one key against one query so the running max jumps mid-way (online-softmax rescale branch)
    if Tk > 70:
        k[:, 70, :d] = q[:, 0, :d] * 4.0
    split = lambda t: t.view(B, -1, Hh, d).permute(0, 2, 1, 3)
    sim = torch.matmul(split(q), split(k).transpose(-1, -2)) * d ** -0.5
    ref = torch.matmul(sim.softmax(-1), split(v)).permute(0, 2, 1, 3).reshape(B, T, Cc)
    Tkp = (Tk + 63) // 64 * 64
    vt = torch.zeros(B, Cc, Tkp, dtype=torch.half)      # pad columns Tk <= t < Tkp zero: the engine's contract for V^T
    vt[:, :, :Tk] = v.permute(0, 2, 1).half()
    out = guarded_out((B, T, Cc), torch.half)
    # Q rows past T and K rows past Tk (of the last sample) sit in NaN guards: the kernels clamp those reads to the last valid row
    qd, kd, vtd = din(q.half()), din(k.half()), din(vt)
    rc = lib.fgdm_op_attention(_p(qd), Cc, _p(kd), Cc, _p(vtd), Tkp, _p(out.t), Cc, B, Hh, T, Tk, d, _st())
    assert rc == 0
    # the kernel the case comments speak of is the kernel that ran (tests/attention_dispatch.py restates the dispatch rules)
    assert lib.fgdm_debug_last_attention_kernel() == expected_kernel(T, Tk, d), case
    torch.cuda.synchronize()
    assert relerr(out.check().float().cpu(), ref) < TOL
    # P is rounded to fp16 before the PV product: blockwise 2 x the normwise bar (= LOCAL_TOL)
    close(f'attention B{B} H{Hh} T{T} Tk{Tk} d{d}', out.t.reshape(B * T, Cc), ref.reshape(B * T, Cc), local=2 * TOL)


def test_sampler_kernels(lib):
    from fgdm_amd import engine as E
    n = (2, 4, 64, 64)
    x, ec, eu, nz = (rnd(n, s).cuda() for s in (51, 52, 53, 54))
    a_t, a_prev, sig = 0.31, 0.42, 0.05
    s1m = float(np.sqrt(1 - a_t))
    x_prev, pred = E.ddim_step(x, ec, eu, 7.5, a_t, a_prev, sig, s1m, nz)
    e = eu + 7.5 * (ec - eu)
    p0 = (x - s1m * e) / np.sqrt(a_t)
    xp = np.sqrt(a_prev) * p0 + np.sqrt(1 - a_prev - sig ** 2) * e + sig * nz
    assert relerr(pred.cpu(), p0.cpu()) < 1e-6 and relerr(x_prev.cpu(), xp.cpu()) < 1e-6
    assert relerr(E.cfg_combine(ec, eu, 9.0).cpu(), (eu + 9.0 * (ec - eu)).cpu()) < 1e-6
    olds = [rnd(n, 60 + i).cuda() for i in range(3)]
    assert relerr(E.plms_combine(ec, olds[-1:]).cpu(), ((3 * ec - olds[-1]) / 2).cpu()) < 1e-6
    assert relerr(E.plms_combine(ec, olds[-2:]).cpu(), ((23 * ec - 16 * olds[-1] + 5 * olds[-2]) / 12).cpu()) < 1e-6
    assert relerr(E.plms_combine(ec, olds).cpu(), ((55 * ec - 59 * olds[-1] + 37 * olds[-2] - 9 * olds[-3]) / 24).cpu()) < 1e-6
    assert relerr(E.axpby(x, 0.5, ec, 0.5).cpu(), ((x + ec) / 2).cpu()) < 1e-6
    got = E.ancestral_step(x, ec, 1.7, 1.3, 0.2, 0.8, 0.4, nz)
    x0 = 1.7 * x - 1.3 * ec
    assert relerr(got.cpu(), (0.2 * x0 + 0.8 * x + 0.4 * nz).cpu()) < 1e-6


SAMPLER_TOL = 1e-6        # fp32 in, fp32 out: only the fp32 rounding of the coefficients and of each operation


def _f32_close(what, g, want):
    got = g.check().cpu()
    e = relerr(got, want)
    te = tile_err(got, want, (256,))
    report(f'{what} [tile_err {te:.3e}]', e, SAMPLER_TOL)
    assert e < SAMPLER_TOL, (what, e)
    assert te < 2 * SAMPLER_TOL, (what, 'tile_err', te)


@pytest.mark.parametrize('n', [12345, 2 * 4 * 64 * 64])
def test_sampler_kernels_abi_guarded(lib, n):
    """The fused sampler updates called through the C ABI (not the engine.py wrappers) on guarded fp32 buffers: an odd element
    count, every NULL-argument form of fgdm_ddim_step, float64 references."""
    x, ec, eu, nz = (rnd((n,), s).double() for s in (51, 52, 53, 54))
    m = torch.rand(n, generator=torch.Generator().manual_seed(55)).double()
    olds = [rnd((n,), 60 + i).double() for i in range(3)]
    dx, dec, deu, dnz, dm = (din(t.float()) for t in (x, ec, eu, nz, m))
    dolds = [din(t.float()) for t in olds]
    f32 = lambda: guarded_out((n,), torch.float32)
    a_t, a_prev, sig, cfg = 0.31, 0.42, 0.05, 7.5
    s1m = float(np.sqrt(1 - a_t))
    for use_eu in (True, False):
        for use_nz in (True, False):
            e = eu + cfg * (ec - eu) if use_eu else ec
            p0 = (x - s1m * e) / np.sqrt(a_t)
            xp = np.sqrt(a_prev) * p0 + np.sqrt(1 - a_prev - sig ** 2) * e + (sig * nz if use_nz else 0)
            # all three outputs, then each one alone (the others NULL)
            for want_outs in ((1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
                gs = [f32() if w else None for w in want_outs]
                rc = lib.fgdm_ddim_step(_p(dx), _p(dec), _p(deu if use_eu else None), cfg, a_t, a_prev, sig, s1m,
                                        _p(dnz if use_nz else None), *(_p(None if g is None else g.t) for g in gs), n, _st())
                assert rc == 0
                torch.cuda.synchronize()
                for g, want, name in zip(gs, (xp, p0, e), ('x_prev', 'pred_x0', 'e_out')):
                    if g is not None:
                        _f32_close(f'ddim_step n{n} eu{int(use_eu)} noise{int(use_nz)} {name}', g, want)
    for order in (1, 2, 3):
        o = olds[-order:]
        want = {1: lambda: (3 * ec - o[-1]) / 2, 2: lambda: (23 * ec - 16 * o[-1] + 5 * o[-2]) / 12,
                3: lambda: (55 * ec - 59 * o[-1] + 37 * o[-2] - 9 * o[-3]) / 24}[order]()
        dd = dolds[-order:]
        e1, e2, e3 = dd[-1], dd[-2] if order >= 2 else None, dd[-3] if order >= 3 else None
        g = f32()
        assert lib.fgdm_plms_combine(_p(dec), _p(e1), _p(e2), _p(e3), order, _p(g.t), n, _st()) == 0
        _f32_close(f'plms_combine n{n} order {order}', g, want)
    for with_b in (True, False):
        g = f32()
        assert lib.fgdm_axpby(_p(dx), 0.5, _p(dec if with_b else None), -1.25, _p(g.t), n, _st()) == 0
        _f32_close(f'axpby n{n} b{int(with_b)}', g, 0.5 * x + (-1.25 * ec if with_b else 0))
    g = f32()
    assert lib.fgdm_mask_blend(_p(dx), _p(dec), _p(dm), _p(g.t), n, _st()) == 0
    _f32_close(f'mask_blend n{n}', g, x * m + (1 - m) * ec)
    for use_nz in (True, False):
        g = f32()
        assert lib.fgdm_ancestral_step(_p(dx), _p(dec), 1.7, 1.3, 0.2, 0.8, 0.4, _p(dnz if use_nz else None), _p(g.t), n, _st()) == 0
        x0 = 1.7 * x - 1.3 * ec
        _f32_close(f'ancestral_step n{n} noise{int(use_nz)}', g, 0.2 * x0 + 0.8 * x + (0.4 * nz if use_nz else 0))


# ----------------------------------------------------------------------------- pipelined big-tile kernel (igemm2.hip)
BIG_CASES = [
    # cfg, B, H, W, C0, C1, Cout, ksize, stride, up, act, extras
    (4, 3, 16, 16, 320, 0, 320, 3, 1, 0, 0, 'cfg4 conv + rowvec + resid, M tail'),
    (4, 2, 16, 16, 640, 320, 640, 3, 1, 0, 1, 'cfg4 concat + silu'),
    (4, 2, 16, 16, 320, 0, 640, 3, 2, 0, 0, 'cfg4 stride 2'),
    (4, 2, 8, 8, 640, 0, 640, 3, 1, 1, 0, 'cfg4 upsample'),
    (4, 2, 16, 16, 1280, 640, 320, 1, 1, 0, 0, 'cfg4 conv1x1 concat'),
    (6, 3, 8, 8, 320, 0, 1280, 3, 1, 0, 2, 'cfg6 conv relu + rowvec + resid, M tail'),
    (6, 1, 3, 5, 64, 0, 320, 3, 1, 0, 0, 'cfg6 tiny odd image'),
    (6, 2, 8, 8, 1280, 1280, 1280, 3, 1, 0, 0, 'cfg6 decoder concat'),
    (5, 2, 8, 8, 640, 0, 1280, 3, 1, 1, 1, 'cfg5 upsample N=1280 silu'),
    (4, 1, 4, 4, 64, 0, 320, 3, 1, 0, 0, 'cfg4 K=576 (18 stages), single tile'),
    (4, 1, 8, 8, 64, 0, 320, 1, 1, 0, 0, 'cfg4 K=64 (2 stages < ring depth)'),
    (6, 1, 8, 8, 32 * 2, 0, 320, 1, 1, 0, 0, 'cfg6 K=64'),
]
# cfg 4..6 run the 16x16x32 MFMA; cfg 7..9 are the same tiles on the 32x32x16 MFMA (kept for A/B measurements)
BIG_CASES = BIG_CASES + [(c[0] + 3,) + c[1:-1] + (c[-1].replace('cfg%d' % c[0], 'cfg%d(mfma32)' % (c[0] + 3)),) for c in BIG_CASES]
# widths that are not multiples of 320 (AutoencoderKL 128 / 256 / 512, hint block 256): 256x256 and 256x128 tiles
BIG_CASES += [
    (5, 3, 16, 16, 128, 0, 512, 3, 1, 0, 1, 'cfg5 N=512 conv silu + rowvec + resid, M tail'),
    (5, 2, 8, 8, 512, 0, 256, 3, 1, 1, 0, 'cfg5 N=256 upsample'),
    (5, 2, 16, 16, 512, 0, 512, 1, 1, 0, 0, 'cfg5 N=512 conv1x1'),
    (10, 3, 16, 16, 128, 0, 128, 3, 1, 0, 0, 'cfg10 N=128 conv + rowvec + resid, M tail'),
    (10, 2, 8, 8, 256, 0, 128, 3, 1, 1, 1, 'cfg10 N=128 upsample silu'),
    (10, 1, 8, 8, 256, 0, 128, 1, 1, 0, 0, 'cfg10 N=128 conv1x1'),
]


# the halo loop (igemm2.hip PIPE = 2, round 4): stride-1 3x3 convolutions whose row tiles are whole rows of one image -- W = 16 /
# 32 / 64 and H W a multiple of 256 -- on both tile heights (cfg 4: 256 x 320, cfg 6: 128 x 320): image borders on every side of
# a tile, tiles in the middle of an image (top / bottom halo rows from the neighbouring tiles' rows), the virtual concat with
# the source switch inside the K walk, every epilogue kind, several samples; whole 8 x 8 images (with an M tail); 16 x 8 and H W = 128 stay on the per-tap loop
BIG_CASES += [
    (4, 1, 16, 16, 128, 0, 320, 3, 1, 0, 0, 'cfg4 halo 16x16 one tile = one image'),
    (4, 3, 16, 16, 64, 64, 640, 3, 1, 0, 1, 'cfg4 halo 16x16 concat silu + rowvec + resid'),
    (4, 2, 32, 32, 192, 0, 320, 3, 1, 0, 0, 'cfg4 halo 32x32 (4 tiles per image) rowvec + resid'),
    (4, 1, 64, 64, 64, 128, 320, 3, 1, 0, 2, 'cfg4 halo 64x64 (16 tiles) concat relu'),
    (4, 2, 8, 32, 128, 0, 320, 3, 1, 0, 0, 'cfg4 halo 8x32 non-square, tile = image'),
    (4, 1, 4, 64, 64, 0, 320, 3, 1, 0, 0, 'cfg4 halo 4x64, tile = image'),
    (6, 2, 16, 16, 192, 0, 320, 3, 1, 0, 1, 'cfg6 halo 16x16 (2 tiles per image) silu + rowvec + resid'),
    (6, 1, 32, 32, 64, 64, 640, 3, 1, 0, 0, 'cfg6 halo 32x32 concat'),
    (6, 1, 64, 64, 128, 0, 320, 3, 1, 0, 0, 'cfg6 halo 64x64 (2-row tiles) rowvec + resid'),
    (4, 5, 8, 8, 128, 64, 320, 3, 1, 0, 1, 'cfg4 halo 8x8 whole images (4 per tile), M tail, concat silu + rowvec + resid'),
    (6, 3, 8, 8, 192, 0, 640, 3, 1, 0, 0, 'cfg6 halo 8x8 whole images (2 per tile), M tail'),
    (4, 2, 16, 8, 128, 0, 320, 3, 1, 0, 0, 'cfg4 16x8: per-tap loop'),
    (6, 1, 2, 64, 128, 0, 320, 3, 1, 0, 0, 'cfg6 H W = 128: per-tap loop'),
]


@pytest.mark.parametrize('case', BIG_CASES, ids=[c[-1] for c in BIG_CASES])
def test_conv_pipelined_kernel(lib, case):
    cfg = case[0]
    assert lib.fgdm_debug_force_igemm_cfg(cfg) == 0
    try:
        inner = case[1:-1] + (case[-1] + (' rowvec' if 'rowvec' in case[-1] else ''),)
        test_conv(lib, inner)
    finally:
        lib.fgdm_debug_force_igemm_cfg(0)


# the 2-stage kernel's three tiles forced (cfg 1 / 2 / 3: 128x128, 128x64, 64x64; the dispatcher picks 2 and 3 by itself) with
# M one row short of and one row past a tile, and widths that are not a multiple of the tile width
TWO_STAGE_CONV_CASES = [
    (1, 1, 127, 1, 64, 0, 96, 3, 1, 0, 0, 'cfg1 M=127 N=96'),
    (1, 3, 43, 1, 64, 0, 4, 3, 1, 0, 1, 'cfg1 M=129 N=4 silu'),
    (2, 1, 127, 1, 64, 64, 192, 3, 1, 0, 0, 'cfg2 M=127 N=192 concat'),
    (2, 3, 43, 1, 128, 0, 96, 3, 1, 0, 0, 'cfg2 M=129 N=96 rowvec + resid'),
    (3, 1, 7, 9, 64, 0, 4, 3, 1, 0, 0, 'cfg3 M=63 N=4'),
    (3, 1, 5, 13, 128, 0, 192, 3, 1, 0, 2, 'cfg3 M=65 N=192 relu rowvec + resid'),
]


@pytest.mark.parametrize('case', TWO_STAGE_CONV_CASES, ids=[c[-1] for c in TWO_STAGE_CONV_CASES])
def test_conv_two_stage_tiles(lib, case):
    test_conv_pipelined_kernel(lib, case)


TWO_STAGE_BM = {1: 128, 2: 128, 3: 64}


@pytest.mark.parametrize('cfg', [1, 2, 3])
def test_linear_two_stage_tile_edges(lib, cfg):
    BM, K = TWO_STAGE_BM[cfg], 320
    x = h16(rnd((BM + 1, K), 81))
    xd = din(x.half())
    try:
        lib.fgdm_debug_force_igemm_cfg(cfg)
        for N in (4, 96, 192):
            w, b = h16(rnd((N, K), 82, 1 / np.sqrt(K))), rnd((N,), 83, 0.1)
            wd, bd = w.cuda(), b.cuda()
            for M in (BM - 1, BM + 1):
                res = h16(rnd((M, N), 84))
                resd = din(res.half())
                out = guarded_out((M, N), torch.half)
                assert lib.fgdm_op_linear(_p(xd), _p(wd), _p(bd), _p(resd), M, K, N, 0, 0, 0, 0, _p(out.t), _st()) == 0
                ref = h16(h16(F.linear(x[:M], w, b)) + res)
                assert relerr(out.check().float().cpu(), ref) < TOL, (M, N)
                close(f'2-stage linear cfg {cfg} M{M} N{N}', out.t, ref)
    finally:
        lib.fgdm_debug_force_igemm_cfg(0)


# pipelined tiles (cfg & 15 -> tile height x width) and their phase-locked K loop (+16)
PIPE_TILES = {4: (256, 320), 5: (256, 256), 6: (128, 320), 10: (256, 128), 11: (64, 160)}


@pytest.mark.parametrize('cfg', [c + p for p in (0, 16) for c in PIPE_TILES])
def test_linear_pipelined_tile_edges(lib, cfg):
    """M one row short of a tile, one row past it, and three tiles plus 17 rows, with a residual, on two column tiles: the ragged
    last row tile of every pipelined tile shape"""
    BM, BN = PIPE_TILES[cfg & 15]
    K, N = 320, 2 * BN
    w, b = h16(rnd((N, K), 85, 1 / np.sqrt(K))), rnd((N,), 86, 0.1)
    wd, bd = w.cuda(), b.cuda()
    try:
        lib.fgdm_debug_force_igemm_cfg(cfg)
        for M in (BM - 1, BM + 1, 3 * BM + 17):
            x, res = h16(rnd((M, K), 87)), h16(rnd((M, N), 88))
            xd, resd = din(x.half()), din(res.half())
            out = guarded_out((M, N), torch.half)
            assert lib.fgdm_op_linear(_p(xd), _p(wd), _p(bd), _p(resd), M, K, N, 0, 0, 0, 0, _p(out.t), _st()) == 0
            ref = h16(h16(F.linear(x, w, b)) + res)
            assert relerr(out.check().float().cpu(), ref) < TOL, M
            close(f'pipelined linear cfg {cfg} M{M}', out.t, ref)
    finally:
        lib.fgdm_debug_force_igemm_cfg(0)


@pytest.mark.parametrize('cfg', [c + p for p in (0, 16) for c in PIPE_TILES])
def test_linear_pipelined_short_k(lib, cfg):
    """The drain of the pipelined K loop: K = 64 is two K-steps (no step refills, two of the three draining arms), K = 128 four
    (one refilling step -- an odd count, so the fragment double buffer changes sides -- then all three draining arms), K = 192 six
    (the two-step loop once, then the odd one).  This entry takes K in multiples of 64 only, so one and three K-steps and an even
    count of refilling steps (K-steps minus three) are reached through split K alone.  One column tile, one row past a row tile."""
    BM, BN = PIPE_TILES[cfg & 15]
    M, N = BM + 1, BN
    res = h16(rnd((M, N), 93))
    resd = din(res.half())
    try:
        lib.fgdm_debug_force_igemm_cfg(cfg)
        for K in (64, 128, 192):
            x, w, b = h16(rnd((M, K), 90)), h16(rnd((N, K), 91, 1 / np.sqrt(K))), rnd((N,), 92, 0.1)
            xd, wd, bd = din(x.half()), w.cuda(), b.cuda()
            out = guarded_out((M, N), torch.half)
            assert lib.fgdm_op_linear(_p(xd), _p(wd), _p(bd), _p(resd), M, K, N, 0, 0, 0, 0, _p(out.t), _st()) == 0
            ref = h16(h16(F.linear(x, w, b)) + res)
            assert relerr(out.check().float().cpu(), ref) < TOL, K
            close(f'pipelined linear cfg {cfg} K{K}', out.t, ref)
    finally:
        lib.fgdm_debug_force_igemm_cfg(0)


@pytest.mark.parametrize('N', [4, 320, 1280])
def test_linear_f32_nchw_output(lib, N):
    """out_kind 2 (OUT_F32_NCHW): the UNet's eps, the ControlNet residuals of the inspection entry and the VAE output leave the
    GEMM epilogue as fp32 [B][N][rows_per_sample] (ld_out = HW).  N = 4 runs on the 2-stage kernel (the UNet's out conv); the
    vector path (rows_per_sample % 4 == 0) and a ragged sample length whose boundaries fall inside row tiles; automatic tile,
    forced cfg 1 and a pipelined tile."""
    K = 320
    w, b = h16(rnd((N, K), 75, 1 / np.sqrt(K))), rnd((N,), 76, 0.1)
    wd, bd = w.cuda(), b.cuda()
    cfgs = (0, 1, 6) if N % 320 == 0 else (0, 1)
    try:
        for rps, Bt in ((100, 3), (77, 3)):
            Mt = rps * Bt
            x = h16(rnd((Mt, K), 77))
            xd = din(x.half())
            want = F.linear(x, w, b).view(Bt, rps, N).permute(0, 2, 1)
            for cfg in cfgs:
                lib.fgdm_debug_force_igemm_cfg(cfg)
                out = guarded_out((Bt, N, rps), torch.float32)
                assert lib.fgdm_op_linear(_p(xd), _p(wd), _p(bd), None, Mt, K, N, 0, 2, rps, rps, _p(out.t), _st()) == 0
                assert relerr(out.check().cpu(), want) < 2e-5, (cfg, rps)
                # fp32 store: blockwise 2 x the normwise bar
                close(f'linear fp32 NCHW N{N} rps {rps} cfg {cfg}', out.t.reshape(-1, rps), want.reshape(-1, rps), 2e-5, 2 * 2e-5)
    finally:
        lib.fgdm_debug_force_igemm_cfg(0)


@pytest.mark.parametrize('N', [320, 1280])
def test_linear_f16_transposed_output_on_pipelined_tiles(lib, N):
    """out_kind 3 (OUT_F16_T) as the FIRST destination at real batch sizes: the cross-attention to_v over the text context
    (Engine::cross_kv, rows_per_sample = 77) and the first-stage AttnBlock's v leave the GEMM as fp16 [B][N][ld], ld =
    roundup(rows_per_sample, 64), by the pipelined kernel's direct 2-byte stores (PATH 0, phase-locked K loop) once the batch is
    large enough for its tiles.  Ragged sample lengths whose boundaries fall inside row tiles (77), the 2-stage kernel's vector path
    (100) and a length with no pad column (64); automatic tile, the 2-stage kernel, 256x320 / 128x320 / 64x160 tiles, 128x320 on the
    phase-locked loop by request and, where N % 256 == 0, 256x256.  float64 reference; the pad columns stay untouched; every
    configuration gives the same bits."""
    K = 320
    w, b = h16(rnd((N, K), 95, 1 / np.sqrt(K))), rnd((N,), 96, 0.1)
    wd, bd = w.cuda(), b.cuda()
    cfgs = (0, 1, 4, 6, 11, 6 + 16) + ((5,) if N == 1280 else ())
    try:
        for rps, Bt in ((77, 5), (100, 3), (64, 5)):
            Mt = rps * Bt
            ld = (rps + 63) // 64 * 64
            x = h16(rnd((Mt, K), 97))
            xd = din(x.half())
            want = F.linear(x.double(), w.double(), b.double()).view(Bt, rps, N).permute(0, 2, 1).reshape(-1, rps).cuda()
            outs = {}
            for cfg in cfgs:
                lib.fgdm_debug_force_igemm_cfg(cfg)
                outT = guarded_out((Bt, N, ld), torch.half)
                assert lib.fgdm_op_linear(_p(xd), _p(wd), _p(bd), None, Mt, K, N, 0, 3, rps, ld, _p(outT.t), _st()) == 0, (cfg, rps)
                torch.cuda.synchronize()
                check_transposed(outT, rps, ld)
                close(f'linear V^T first destination N{N} rps {rps} cfg {cfg}', outT.t[:, :, :rps].reshape(-1, rps), want)
                outs[cfg] = outT.t[:, :, :rps]
            for cfg in cfgs[1:]:
                assert torch.equal(outs[0], outs[cfg]), f'N{N} rps {rps}: automatic tile and cfg {cfg} differ'
    finally:
        lib.fgdm_debug_force_igemm_cfg(0)


@pytest.mark.parametrize('M', [154, 201])
def test_linear_quick_gelu(lib, M):
    """act 4, x sigmoid(1.702 x): the CLIP MLP's first projection (768 -> 3072, M = 2 x 77 tokens, and a ragged M); only the
    2-stage kernel carries it"""
    K, N = 768, 3072
    x = h16(rnd((M, K), 78))
    w, b = h16(rnd((N, K), 79, 1 / np.sqrt(K))), rnd((N,), 80, 0.1)
    y = F.linear(x, w, b)
    ref = y * torch.sigmoid(1.702 * y)
    xd, wd, bd = din(x.half()), w.cuda(), b.cuda()
    out = guarded_out((M, N), torch.half)
    assert lib.fgdm_op_linear(_p(xd), _p(wd), _p(bd), None, M, K, N, 4, 0, 0, 0, _p(out.t), _st()) == 0
    assert relerr(out.check().float().cpu(), ref) < TOL
    close(f'linear quick-GELU M{M}', out.t, ref)


def test_long_k_linear_at_8_prompts_same_bits_on_every_tile(lib):
    """The 16x16 level's feed-forward output at 8 prompts per GPU (M = 4096, K = 5120 -> 1280, + residual; attention.py:53-64): the
    automatic choice (256x128 tiles, round 4) against torch, and bit for bit against 128x320, 64x160 and the 2-stage kernel --
    which tile runs depends on the batch, a sample's result must not."""
    M, K, N = 4100, 5120, 1280
    x = h16(rnd((M, K), 91))
    w, b = h16(rnd((N, K), 92, 1 / np.sqrt(K))), rnd((N,), 93, 0.1)
    res = h16(rnd((M, N), 94))
    xd, wd, bd, rd = din(x.half()), w.cuda(), b.cuda(), din(res.half())
    ref = h16(h16(F.linear(x, w, b)) + res)
    outs = {}
    try:
        for cfg in (0, 6, 10, 11, 1):
            lib.fgdm_debug_force_igemm_cfg(cfg)
            out = guarded_out((M, N), torch.half)
            assert lib.fgdm_op_linear(_p(xd), _p(wd), _p(bd), _p(rd), M, K, N, 0, 0, 0, 0, _p(out.t), _st()) == 0
            assert relerr(out.check().float().cpu(), ref) < TOL, cfg
            close(f'long-K linear cfg {cfg}', out.t, ref)
            outs[cfg] = out.t
    finally:
        lib.fgdm_debug_force_igemm_cfg(0)
    for cfg in (6, 10, 11, 1):
        assert torch.equal(outs[0], outs[cfg]), f'automatic tile and cfg {cfg} differ'


def test_linear_pipelined_kernel(lib):
    try:
        M, K = 300, 320
        x = h16(rnd((M, K), 71))
        xd = din(x.half())
        # GEGLU through the 256x256 configuration
        N = 2560
        w, b = h16(rnd((N, K), 72, 1 / np.sqrt(K))), rnd((N,), 73, 0.1)
        y = F.linear(x, w, b)
        a, g = y.chunk(2, dim=-1)
        wd, bd = w.cuda(), b.cuda()
        for cfg in (5, 8):
            lib.fgdm_debug_force_igemm_cfg(cfg)
            out = guarded_out((M, N // 2), torch.half)
            assert lib.fgdm_op_linear(_p(xd), _p(wd), _p(bd), None, M, K, N, 3, 0, 0, 0, _p(out.t), _st()) == 0
            assert relerr(out.check().float().cpu(), a * F.gelu(g)) < TOL, cfg
            close(f'pipelined GEGLU cfg {cfg}', out.t, a * F.gelu(g))
        # plain / fp32 / transposed outputs through 256x320 and 128x320
        N2 = 640
        w2, b2 = w[:N2].contiguous(), b[:N2].contiguous()
        w2d, b2d = w2.cuda(), b2.cuda()
        ref = F.linear(x, w2, b2)
        res = h16(rnd((M, N2), 74))
        resd = din(res.half())
        for cfg in (4, 6, 7, 9, 11, 27):      # 11 / 27: the four-wave 64x160 tile, pipelined / phase-locked K loop
            lib.fgdm_debug_force_igemm_cfg(cfg)
            out = guarded_out((M, N2), torch.half)
            assert lib.fgdm_op_linear(_p(xd), _p(w2d), _p(b2d), _p(resd), M, K, N2, 0, 0, 0, 0, _p(out.t), _st()) == 0
            assert relerr(out.check().float().cpu(), ref + res) < TOL, cfg
            close(f'pipelined linear + resid cfg {cfg}', out.t, ref + res)
            out32 = guarded_out((M, N2), torch.float32)
            assert lib.fgdm_op_linear(_p(xd), _p(w2d), _p(b2d), None, M, K, N2, 0, 1, 0, 0, _p(out32.t), _st()) == 0
            assert relerr(out32.check().cpu(), ref) < 2e-5, cfg
            close(f'pipelined linear fp32 cfg {cfg}', out32.t, ref, 2e-5, 2 * 2e-5)     # fp32 store: 2 x the normwise bar
            for rps, Bt in ((100, 3), (77, 2)):
                Mt = rps * Bt
                ld = (rps + 63) // 64 * 64
                outT = guarded_out((Bt, N2, ld), torch.half)
                xt = din(x[:Mt].half())
                assert lib.fgdm_op_linear(_p(xt), _p(w2d), _p(b2d), None, Mt, K, N2, 0, 3, rps, ld, _p(outT.t), _st()) == 0
                want = ref[:Mt].view(Bt, rps, N2).permute(0, 2, 1)
                check_transposed(outT, rps, ld)
                assert relerr(outT.t[:, :, :rps].float().cpu(), want) < TOL, (cfg, rps)
                close(f'pipelined V^T cfg {cfg} rps {rps}', outT.t[:, :, :rps].reshape(-1, rps), want.reshape(-1, rps))
    finally:
        lib.fgdm_debug_force_igemm_cfg(0)


@pytest.mark.parametrize('knob', ['FGDM_ATTN_DQ=1', 'FGDM_ATTN_DQ=0 FGDM_ATTN_DQ80=0'])
def test_attention_alternative_kernels(knob):
    """The kernels the default path no longer takes for the self-attention shapes -- the 16-wide form of the two-strand kernel
    (FGDM_ATTN_DQ=1: faster on random operands, slower inside the network) and the ping-pong kernel for every long shape
    (FGDM_ATTN_DQ=0 FGDM_ATTN_DQ80=0) -- stay selectable for same-box A/B runs, so they stay under the same parity cases.  The knobs
    are read once per process: a fresh interpreter runs the attention cases under each."""
    import os
    import subprocess
    import sys
    env = dict(os.environ)
    for kv in knob.split():
        k, v = kv.split('=')
        env[k] = v
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-q', '-x', '-m', 'gpu', '-k',
                        'test_attention and not alternative'], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]


@pytest.mark.parametrize('gain,shift', [(6.0, 0.0), (3.0, 2.0), (0.05, 0.0)], ids=['large logits', 'all-negative rows', 'flat rows'])
def test_attention_logit_ranges_d40(lib, gain, shift):
    """d = 40 keeps the softmax scale and the running max inside the QK^T MFMA (fp16 Q pad slot): logits spanning
    hundreds of log2 units, rows whose logits are all strongly negative (first tile must still set the offset) and
    almost flat rows must all stay within the per-kernel tolerance."""
    B, Hh, T, Tk, d = 1, 2, 256, 320, 40
    Cc = Hh * d
    q, k, v = h16(rnd((B, T, Cc), 71) * gain), h16(rnd((B, Tk, Cc), 72) * gain), h16(rnd((B, Tk, Cc), 73))
    if shift:
        q, k = h16(q.abs() + shift), h16(-(k.abs() + shift))        # every q.k strongly negative
    split = lambda t: t.view(B, -1, Hh, d).permute(0, 2, 1, 3)
    sim = torch.matmul(split(q).double(), split(k).double().transpose(-1, -2)) * d ** -0.5
    ref = torch.matmul(sim.softmax(-1), split(v).double()).permute(0, 2, 1, 3).reshape(B, T, Cc)
    vt = v.permute(0, 2, 1).half().contiguous()
    out = guarded_out((B, T, Cc), torch.half)
    qd, kd, vtd = din(q.half()), din(k.half()), din(vt)
    assert lib.fgdm_op_attention(_p(qd), Cc, _p(kd), Cc, _p(vtd), Tk, _p(out.t), Cc, B, Hh, T, Tk, d, _st()) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out.check()).all()
    assert relerr(out.t.float().cpu(), ref) < 2 * TOL, float(sim.abs().max())
    # fp16 P over logits spanning hundreds of log2 units: blockwise 2 x this family's normwise bar
    close(f'attention logit range gain {gain:g} shift {shift:g}', out.t.reshape(B * T, Cc), ref.reshape(B * T, Cc), 2 * TOL, 4 * TOL)


# M, K1, C, N2, act2 (0 / 3 = GEGLU), resid, forced tile cfg (0 = automatic), expected partial-sum slots per row (< 0: from
# the separate row-statistics pass instead of the producing GEMM's epilogue)
LN_CASES = [
    (32768, 320, 320, 640, 0, True, 0, 2),      # 128x320 pipelined tiles: statistics from the producer's epilogue (2 slots)
    (16384, 320, 320, 640, 0, True, 0, 2),      # 128 tiles of 128x320 would fill half the chip: 64x160 four-wave tiles (round 4); the two
                                                # 80-column waves of a row meet in LDS and write the same 160-column slots, same bits
    (65536, 320, 320, 2560, 3, True, 0, 2),     # 256x320 producer, GEGLU consumer on 256x256 tiles
    (8192, 1280, 1280, 1280, 0, True, 0, 8),    # 8 slots per row
    (8192, 640, 640, 5120, 3, False, 0, 4),     # producer: 64x160 tiles (128 tiles of 128x320 = half the chip); consumer: persistent GEGLU kernel
    (32768, 640, 640, 5120, 3, False, 0, 4),    # producer on 128x320 tiles: 4 slots from its epilogue
    (16500, 640, 640, 5120, 3, True, 0, 4),     # ragged M through the persistent GEGLU kernel (65 row tiles x 20 column tiles)
    (200, 320, 320, 320, 0, True, 0, -2),       # small problem: 2-stage kernel + the separate row-statistics pass (same 2 slots)
    (16384, 320, 320, 640, 0, True, 1, -2),     # the same shape as case 0 forced onto the 2-stage kernel
    (4100, 640, 640, 640, 0, False, 6, 4),      # ragged M on the 128x320 tiles
    (8192, 1280, 1280, 3840, 0, True, 0, 8),    # the 16x16 level's q|k|v width: 256x256 tiles divide the chip better (automatic)
    (2048, 1280, 1280, 1280, 0, True, 0, 8),    # the 8x8 level: 64x160 four-wave tiles (automatic), statistics from their epilogue
    (4100, 1280, 1280, 1280, 0, True, 0, 8),    # ragged M on the 64x160 tiles (the 16x16 level at 8 prompts per GPU, plus four rows)
    (2050, 1280, 1280, 1280, 0, True, 27, 8),   # the 64x160 tile on the phase-locked K loop emits them the same way
    (6600, 320, 320, 2560, 3, True, 0, 2),      # the smallest consumer on the persistent GEGLU kernel: 26 row tiles (the last ragged) x 10
                                                # column tiles = 260 > 256 (test_persistent_walk_modes runs it under both tile walks)
]


@pytest.mark.parametrize('case', LN_CASES, ids=lambda c: f'M{c[0]}_K{c[1]}_C{c[2]}_N{c[3]}_act{c[4]}_cfg{c[6]}')
def test_layernorm_folded_into_consumer_gemm(lib, case):
    """The transformer block's LayerNorms (attention.py:234-240) never run as kernels: the producing GEMM leaves per-row partial
    sums next to its output, the consuming GEMM multiplies the raw tokens with gamma-folded weights and applies (mean, rstd)
    to its fp32 accumulator.  Reference arithmetic: fp16 h as stored, then nn.LayerNorm + nn.Linear (+ GEGLU) in fp32 on the
    fp16-rounded folded weights."""
    M, K1, Cc, N2, act2, use_res, cfg, want_slots = case
    x = rnd((M, K1), 1).half()
    w1, b1 = rnd((Cc, K1), 2, K1 ** -0.5), rnd((Cc,), 3, 0.1)
    res = rnd((M, Cc), 4).half() if use_res else None
    gamma, beta = 1.0 + 0.2 * rnd((Cc,), 5), 0.1 * rnd((Cc,), 6) + 0.05
    w2, b2 = rnd((N2, Cc), 7, Cc ** -0.5), rnd((N2,), 8, 0.1)
    nout = N2 // 2 if act2 == 3 else N2
    gh = guarded_out((M, Cc), torch.float16)
    gy = guarded_out((M, nout), torch.float16)
    h, y = gh.t, gy.t
    slots = C.c_int(0)
    dev = lambda t: None if t is None else t.cuda()
    xs, rs, ws = din(x), (None if res is None else din(res)), [dev(t) for t in (w1, b1, gamma, beta, w2, b2)]
    try:
        lib.fgdm_debug_force_igemm_cfg(cfg)
        rc = lib.fgdm_op_linear_ln_linear(_p(xs), _p(ws[0]), _p(ws[1]), _p(rs), _p(ws[2]), _p(ws[3]), _p(ws[4]), _p(ws[5]), M, K1, Cc,
                                          N2, act2, _p(h), _p(y), C.byref(slots), _st())
    finally:
        lib.fgdm_debug_force_igemm_cfg(0)
    assert rc == 0
    assert slots.value == want_slots
    gh.check()
    gy.check()
    # producer: fp16 GEMM result, then the fp16 residual added and rounded (the engine's policy)
    h_ref = h16(F.linear(x.float(), h16(w1), b1))
    if use_res:
        h_ref = h16(h_ref + res.float())
    assert relerr(h.float().cpu(), h_ref) < TOL
    close(f'LayerNorm fold producer M{M} C{Cc} cfg {cfg}', h, h_ref)
    # consumer on the engine's OWN h (so that only the folded LayerNorm + GEMM is judged)
    hh = h.float().cpu()
    wf = h16(w2 * gamma[None, :])
    cb = w2 @ beta + b2
    z = F.linear(F.layer_norm(hh, (Cc,), None, None, 1e-5), wf, cb)
    if act2 == 3:
        a, g = z.chunk(2, dim=-1)
        z = a * F.gelu(g)
    assert relerr(y.float().cpu(), h16(z)) < TOL
    close(f'LayerNorm fold consumer M{M} C{Cc} N{N2} act{act2} cfg {cfg}', y, h16(z))
    if cfg == 0:      # the same problem forced onto the 2-stage kernels (+ the separate statistics pass): not a bit may differ --
        gh2 = guarded_out((M, Cc), torch.float16)      # which kernel evaluates a layer depends on the batch size, a sample's
        gy2 = guarded_out((M, nout), torch.float16)    # result must not
        h2, y2 = gh2.t, gy2.t
        try:
            lib.fgdm_debug_force_igemm_cfg(1)
            assert lib.fgdm_op_linear_ln_linear(_p(xs), _p(ws[0]), _p(ws[1]), _p(rs), _p(ws[2]), _p(ws[3]), _p(ws[4]), _p(ws[5]), M,
                                                K1, Cc, N2, act2, _p(h2), _p(y2), C.byref(slots), _st()) == 0
        finally:
            lib.fgdm_debug_force_igemm_cfg(0)
        assert slots.value == -abs(want_slots)
        gh2.check()
        gy2.check()
        assert torch.equal(h2, h), 'producer output differs between kernels'
        assert torch.equal(y2, y), 'LayerNorm-folded consumer output differs between kernels'
    # ... which is the reference's LayerNorm -> Linear up to the fp16 rounding of the weights
    z32 = F.linear(F.layer_norm(hh, (Cc,), gamma, beta, 1e-5), w2, b2)
    if act2 == 3:
        a, g = z32.chunk(2, dim=-1)
        z32 = a * F.gelu(g)
    assert relerr(y.float().cpu(), z32) < TOL


@pytest.mark.parametrize('mode', ['2', '0'])
def test_persistent_walk_modes(mode):
    """FGDM_IGEMM_PERSIST=2 (contiguous runs instead of the default round-robin walk) and =0 (one workgroup per tile) stay selectable
    for same-box A/B runs, so they stay under the same cases.  With 260 tiles, mode 2 gives the workgroups of four XCDs runs of two
    tiles: some stay in one row block (the next tile's (mean, rstd) are COPIED from the other operand set), some cross into the next
    (they are recomputed); the LayerNorm case holds either bitwise against the 2-stage kernel.  The knob is read once per process:
    a fresh interpreter runs that case and the smaller persistent-kernel case under each value."""
    import os
    import subprocess
    import sys
    env = dict(os.environ, FGDM_IGEMM_PERSIST=mode)
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-q', '-x', '-m', 'gpu', '-k',
                        '(test_layernorm_folded_into_consumer_gemm and M6600_) or (test_geglu_persistent_kernel and L1)'],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    assert '2 passed' in r.stdout, r.stdout[-3000:]


@pytest.mark.parametrize('offset', [8.0, 32.0], ids=lambda o: f'row_mean_{int(o)}_std')
def test_layernorm_fold_rows_with_large_mean(lib, offset):
    """the folded LayerNorm takes its variance as E[x^2] - mean^2 from fp32 partial sums and forms acc - mean u in fp32;
    both cancel when |mean| >> std.  Token rows shifted by `offset` standard deviations plus a few outlier channels (what real
    checkpoints produce) must stay inside the per-kernel bar -- measured against LayerNorm -> Linear in fp64 ON THE ENGINE'S OWN
    fp16 h (the fp16 storage of a row with a large mean loses the same bits in the reference's autocast path)."""
    M, K1, Cc, N2 = 4096, 320, 320, 640
    x = rnd((M, K1), 1).half()
    w1, b1 = rnd((Cc, K1), 2, K1 ** -0.5), rnd((Cc,), 3, 0.1)
    res = rnd((M, Cc), 4) + offset * (0.5 + rnd((M, 1), 9).abs())          # row means of 0.5 ... 1.5 x offset, unit spread
    res[:, ::97] += 6.0 * rnd((M, Cc), 10)[:, ::97]                         # four outlier channels
    res = res.half()
    gamma, beta = 1.0 + 0.2 * rnd((Cc,), 5), 0.1 * rnd((Cc,), 6) + 0.05
    w2, b2 = rnd((N2, Cc), 7, Cc ** -0.5), rnd((N2,), 8, 0.1)
    gh = guarded_out((M, Cc), torch.float16)
    gy = guarded_out((M, N2), torch.float16)
    slots = C.c_int(0)
    ws = [t.cuda() for t in (w1, b1, gamma, beta, w2, b2)]
    xd, rd = din(x), din(res)
    rc = lib.fgdm_op_linear_ln_linear(_p(xd), _p(ws[0]), _p(ws[1]), _p(rd), _p(ws[2]), _p(ws[3]), _p(ws[4]), _p(ws[5]), M,
                                      K1, Cc, N2, 0, _p(gh.t), _p(gy.t), C.byref(slots), _st())
    assert rc == 0
    gh.check()
    y = gy.check()
    hh = gh.t.double().cpu()
    wf = h16(w2 * gamma[None, :]).double()
    z = F.linear(F.layer_norm(hh, (Cc,), None, None, 1e-5), wf, (w2.double() @ beta.double() + b2.double()))
    err = relerr(y.double().cpu(), z)
    print(f'LayerNorm fold, row mean ~{offset:g} x std: rel_err={err:.3e}')
    assert err < TOL
    close(f'LayerNorm fold, row mean ~{offset:g} x std', y, z)
