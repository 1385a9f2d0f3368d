"""Per-kernel parity for the stacked q | k | v projection of every self-attention (Engine::attn_fwd, csrc/engine.hip): ONE LINEAR
GEMM over the raw tokens h with norm1 folded in and two destinations -- packed columns [0, 2C) row-major to qk [B T, 2C], columns
[2C, 3C) TRANSPOSED to vt [B, C, Tp] (IgemmArgs::out2, OUT_F16_T, ld_out2 = Tp = roundup(T, 64), split_n = 2C, rows_per_sample =
T) -- through the diagnostic entry fgdm_op_ln_qkv, which launches it with exactly those fields.

Three epilogues can write that V^T; which one runs depends on the geometry and on the tile the batch size selects:
  staged   igemm2.hip PATH 1 of the LayerNorm consumers (TR): [channel][32 tokens] in LDS, 16-byte runs along the token axis.
           Needs the fold, T % 32 == 0, M % 32 == 0, Tp % 8 == 0 and a 16-byte aligned vt (epilogue_path).
  direct   igemm2.hip PATH 0, 2-byte stores, on the phase-locked K loop: any other T, and every fold = 0 call.
  2-stage  igemm.hip: the h4 vector path when T % 4 == 0, scalar stores otherwise.
Configuration numbers are fgdm_debug_force_igemm_cfg's: 0 automatic; 1 the 2-stage kernel (128 x 128); 4 / 5 / 6 / 11 the pipelined
256 x 320 / 256 x 256 / 128 x 320 / 64 x 160 tiles; + 16 the phase-locked K loop.  The library has no query for the GEMM kernel
that ran, so the path each line of the log names is the launcher's rule restated here (`path_of`), not a measurement.  At these
sizes the AUTOMATIC choice reaches a pipelined tile only for (B 1, T 1024, C 1280) (128 x 320: 96 tiles); every other shape runs
on the 2-stage kernel by itself, and the forced configurations carry the coverage of the pipelined epilogues.

Reference: float64 on the CPU on the fp16 h as the kernel reads it.  fold = 1: layer_norm(h, eps 1e-5) without affine, times
the fp16-rounded gamma-folded stacked weight, plus W beta (what the packer builds; the result is NOT rounded to fp16 again), and --
normwise, at the same bar -- the reference's own LayerNorm(gamma, beta) -> Linear with the unrounded weights.  fold = 0: a plain
linear on the fp16-rounded weights.  V^T is compared as [B C, T] rows, so tile_err's 32 x 32 blocks follow the store layout.
Bars: the project's own, normwise TOL = 1e-3 and blockwise LOCAL_TOL = 2e-3, separately for q | k and for V^T.

Every call also asserts: guards of qk, vt intact (tests/guarded.py); every element of qk written and finite; every (b, c, t < T)
of vt written and finite; the pad columns [T, Tp) of vt untouched (the engine zeroes them once and relies on the GEMM writing
around them).  A configuration the launcher refuses for a shape (256 x 256 tiles when 3C % 256 != 0) must return FGDM_ERR_ARG with
both outputs untouched.  Which tile runs depends on the batch, a sample's result must not: all configurations that run give the
same bits, and a sample evaluated alone gives the bits of its rows / its V^T plane in the batch.

The measured errors are printed and appended to the file FGDM_QKV_PARITY_LOG names when it is set
(profiles/qkv_projection_parity_errors.txt is a copy of one such run)."""
import ctypes as C
import functools
import os

import pytest
import torch
import torch.nn.functional as F

from guarded import guarded_out
from test_gpu_ops import TOL, _p, _st, close, din, h16, rnd
from common import relerr

pytestmark = pytest.mark.gpu

ERR_ARG = -1
PIPELINED = {4: (256, 320), 5: (256, 256), 6: (128, 320), 11: (64, 160)}
CFGS = (0, 4, 6, 11, 4 + 16, 6 + 16, 11 + 16, 1, 5)

# B, T, C, Tp
STAGED_CASES = [
    (5, 64, 320, 64),          # four samples inside one 256-row tile; ragged last row tile (M = 320)
    (3, 96, 640, 128),         # sample boundaries on 32-row passes that are not tile-aligned; real pad columns
    (3, 256, 320, 256),        # one sample per 256-row tile
    (1, 1024, 1280, 1024),     # several row tiles per sample; 3C % 256 == 0: the only shape the 256 x 256 tile accepts
]
DIRECT_CASES = [
    (3, 100, 320, 128),        # T % 4 == 0: the 2-stage kernel's h4 path
    (7, 25, 1280, 64),         # T % 4 != 0: its scalar path; seven samples inside one tile; M = 175
    (2, 144, 640, 192),
]
UNFOLDED_CASES = [(5, 64, 320, 64), (3, 100, 320, 128)]


@pytest.fixture(scope='module')
def lib():
    from fgdm_amd import _lib
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return _lib.load()


def record(line):
    print(line)
    path = os.environ.get('FGDM_QKV_PARITY_LOG')
    if path:
        with open(path, 'a') as f:
            f.write(line + '\n')


def ident(c):
    return 'B%d_T%d_C%d_Tp%d' % c


def automatic_cfg(M, N):
    """pick_force (igemm.hip) for a LINEAR GEMM with K % 64 == 0, N % 320 == 0, no GEGLU, no long K: 0 = the 2-stage kernel"""
    up = lambda a, b: (a + b - 1) // b
    b256, b128, b64 = up(M, 256) * (N // 320), up(M, 128) * (N // 320), up(M, 64) * (N // 160)
    if b256 >= 192:
        return 4
    if b128 >= 96 and not (b128 < 192 and b64 >= 512):
        return 6
    return 11 if b64 >= 128 else 0


def accepted(cfg, Cc):
    """igemm2_launch refuses a tile whose width does not divide N = 3C (its weight rows are not padded to the tile)"""
    return cfg != 5 or (3 * Cc) % 256 == 0


def path_of(cfg, B, T, Cc, Tp, fold):
    """the kernel and V^T epilogue a configuration takes, by the rules of igemm_launch / igemm2_launch / epilogue_path"""
    M = B * T
    eff = cfg if cfg else automatic_cfg(M, 3 * Cc)
    if eff < 4:
        return '2-stage kernel, V^T by %s' % ('h4 vectors' if T % 4 == 0 else 'scalar stores')
    tile = '%dx%d' % PIPELINED[eff & 15]
    if fold and T % 32 == 0 and M % 32 == 0 and Tp % 8 == 0:
        return 'pipelined %s, %s K loop, PATH 1, V^T staged (16-byte runs)' % (tile, 'phase-locked' if eff & 16 else 'pipelined')
    return 'pipelined %s, phase-locked K loop, PATH 0, V^T direct (2-byte stores)' % tile


def make_h(B, T, Cc, offset=0.0):
    """fp16 tokens [B T, C]; offset: every row shifted by 0.5 ... 1.5 x offset standard deviations plus outlier channels, as in
    test_layernorm_fold_rows_with_large_mean"""
    M = B * T
    h = rnd((M, Cc), 101) * 1.3 + 0.2
    if offset:
        h = rnd((M, Cc), 101) + offset * (0.5 + rnd((M, 1), 109).abs())
        h[:, ::97] += 6.0 * rnd((M, Cc), 110)[:, ::97]
    return h.half()


@functools.lru_cache(maxsize=None)
def weights(Cc):
    """(wq, wk, wv, gamma, beta), fp32 on the host"""
    w = tuple(rnd((Cc, Cc), 102 + i, Cc ** -0.5) for i in range(3))
    return w + (1.0 + 0.2 * rnd((Cc,), 105), 0.1 * rnd((Cc,), 106) + 0.05)


def reference(h, Cc, fold):
    """float64 [M, 3C] (q | k | v) on the DEVICE, and for fold = 1 the unfolded LayerNorm -> Linear next to it (else None)"""
    wq, wk, wv, gamma, beta = weights(Cc)
    W = torch.cat([wq, wk, wv], 0)
    hh = h.double()
    if not fold:
        return F.linear(hh, h16(W).double()).cuda(), None
    wf = h16(W * gamma[None, :]).double()             # the packer's fp32 product, rounded to fp16
    ref = F.linear(F.layer_norm(hh, (Cc,), None, None, 1e-5), wf, W.double() @ beta.double())
    plain = F.linear(F.layer_norm(hh, (Cc,), gamma.double(), beta.double(), 1e-5), W.double())
    return ref.cuda(), plain.cuda()


class Problem:
    """one shape: its input between NaN guards, its weights on the device, its reference (computed once, never modified)"""

    def __init__(self, case, fold, offset=0.0, h=None):
        self.case, self.fold = case, fold
        self.B, self.T, self.C, self.Tp = case
        self.h = make_h(self.B, self.T, self.C, offset) if h is None else h
        self.hd = din(self.h)
        wq, wk, wv, gamma, beta = weights(self.C)
        self.wd = [t.cuda() for t in (wq, wk, wv)]
        self.gd, self.bd = (gamma.cuda(), beta.cuda()) if fold else (None, None)
        self._ref = None

    def ref(self):
        if self._ref is None:
            self._ref = reference(self.h, self.C, self.fold)
        return self._ref

    def run(self, lib, cfg):
        """-> (rc, qk, vt) with every structural assertion of the module docstring made"""
        B, T, Cc, Tp = self.case
        gqk = guarded_out((B * T, 2 * Cc), torch.half)
        gvt = guarded_out((B, Cc, Tp), torch.half)
        try:
            lib.fgdm_debug_force_igemm_cfg(cfg)
            rc = lib.fgdm_op_ln_qkv(_p(self.hd), _p(self.gd), _p(self.bd), _p(self.wd[0]), _p(self.wd[1]), _p(self.wd[2]),
                                    B, T, Cc, Tp, self.fold, _p(gqk.t), _p(gvt.t), _st())
        finally:
            lib.fgdm_debug_force_igemm_cfg(0)
        torch.cuda.synchronize()
        if rc != 0:
            for g in (gqk, gvt):            # a refused launch writes nothing
                g.check_guards()
                g.assert_untouched(None)
            return rc, None, None
        gqk.check()
        valid = (slice(None), slice(None), slice(0, T))
        gvt.check(valid)
        if Tp > T:
            gvt.assert_untouched((slice(None), slice(None), slice(T, None)))
        return rc, gqk.t, gvt.t

    def parity(self, what, qk, vt):
        B, T, Cc, Tp = self.case
        ref, plain = self.ref()
        as_vt = lambda r: r[:, 2 * Cc:].reshape(B, T, Cc).permute(0, 2, 1).reshape(B * Cc, T)
        got_vt = vt[:, :, :T].reshape(B * Cc, T)
        e_qk, te_qk = close(f'{what} q|k', qk, ref[:, :2 * Cc])
        e_vt, te_vt = close(f'{what} V^T', got_vt, as_vt(ref))
        if plain is not None:       # ... which is the reference's LayerNorm -> Linear up to the fp16 rounding of the weights
            assert relerr(qk, plain[:, :2 * Cc]) < TOL, what
            assert relerr(got_vt, as_vt(plain)) < TOL, what
        return e_qk, te_qk, e_vt, te_vt


def run_configurations(lib, prob, cfgs, family):
    """every configuration on one problem: parity for each that runs, FGDM_ERR_ARG with untouched outputs for each the launcher
    refuses, and the same bits from all that run.  Returns {cfg: (qk, vt)}."""
    B, T, Cc, Tp = prob.case
    outs = {}
    for cfg in cfgs:
        rc, qk, vt = prob.run(lib, cfg)
        name = f'{family} {ident(prob.case)} fold {prob.fold} cfg {cfg}'
        if not accepted(cfg & 15 if cfg >= 4 else cfg, Cc):
            assert rc == ERR_ARG, (name, rc)
            record(f'{name}: refused (3C % 256 != 0), FGDM_ERR_ARG, qk and vt untouched')
            continue
        assert rc == 0, (name, rc)
        e_qk, te_qk, e_vt, te_vt = prob.parity(name, qk, vt)
        record(f'{name} [{path_of(cfg, B, T, Cc, Tp, prob.fold)}]: q|k rel_err={e_qk:.3e} tile_err={te_qk:.3e}; '
               f'V^T rel_err={e_vt:.3e} tile_err={te_vt:.3e} bars {TOL:.1e} / 2.0e-03')
        outs[cfg] = (qk, vt)
    first = min(outs)
    for cfg, (qk, vt) in outs.items():
        assert torch.equal(qk, outs[first][0]), f'{ident(prob.case)}: q|k of cfg {cfg} and cfg {first} differ'
        assert torch.equal(vt[:, :, :T], outs[first][1][:, :, :T]), f'{ident(prob.case)}: V^T of cfg {cfg} and cfg {first} differ'
    return outs


@pytest.mark.parametrize('case', STAGED_CASES, ids=ident)
def test_qkv_staged_vt(lib, case):
    """fold = 1, T % 32 == 0: the pipelined tiles stage V^T in LDS and store 16-byte runs along the token axis"""
    B, T, Cc, Tp = case
    assert T % 32 == 0 and (B * T) % 32 == 0
    assert 'staged' in path_of(4, B, T, Cc, Tp, 1) and 'staged' in path_of(11 + 16, B, T, Cc, Tp, 1)
    outs = run_configurations(lib, Problem(case, 1), CFGS, 'staged')
    assert (5 in outs) == (case == (1, 1024, 1280, 1024))


@pytest.mark.parametrize('case', DIRECT_CASES, ids=ident)
def test_qkv_direct_vt(lib, case):
    """fold = 1, T % 32 != 0 (10 x 10, 5 x 5, 12 x 12 latent levels): PATH 0's 2-byte transposed stores on the pipelined tiles, the
    h4 / scalar stores of the 2-stage kernel"""
    B, T, Cc, Tp = case
    assert T % 32 != 0
    assert 'direct' in path_of(4, B, T, Cc, Tp, 1)
    run_configurations(lib, Problem(case, 1), CFGS, 'direct')


@pytest.mark.parametrize('case', UNFOLDED_CASES, ids=ident)
def test_qkv_without_fold(lib, case):
    """fold = 0 (the FGDM_LN_FOLD=0 engine: h already normalised, plain weights, no statistics): the non-LayerNorm instantiations,
    whose PATH 1 has no transposed staging -- V^T always leaves by the direct stores"""
    B, T, Cc, Tp = case
    assert 'direct' in path_of(6, B, T, Cc, Tp, 0)
    run_configurations(lib, Problem(case, 0), (0, 6, 1), 'unfolded')


@pytest.mark.parametrize('offset', [8.0, 32.0], ids=lambda o: f'row_mean_{int(o)}_std')
def test_qkv_rows_with_large_mean(lib, offset):
    """Token rows shifted by `offset` standard deviations (test_layernorm_fold_rows_with_large_mean): the V^T half gets the same
    acc - mean u fix-up as q | k, on the staged, the direct-capable and the 2-stage epilogues"""
    run_configurations(lib, Problem(STAGED_CASES[0], 1, offset), (0, 4, 11, 6 + 16), f'large mean {offset:g} std')


@pytest.mark.parametrize('case', [STAGED_CASES[1], DIRECT_CASES[1]], ids=ident)
def test_qkv_sample_alone_equals_sample_in_batch(lib, case):
    """sample b evaluated alone (B = 1: another grid, another ragged tile, for the staged shape another position of every 32-row
    pass inside its tile) gives the bits of its rows of qk and of its V^T plane in the batch call"""
    B, T, Cc, Tp = case
    batch = Problem(case, 1)
    for cfg in (0, 6):
        rc, qk, vt = batch.run(lib, cfg)
        assert rc == 0
        for b in range(B):
            alone = Problem((1, T, Cc, Tp), 1, h=batch.h[b * T:(b + 1) * T].clone())
            rc1, qk1, vt1 = alone.run(lib, cfg)
            assert rc1 == 0
            assert torch.equal(qk1, qk[b * T:(b + 1) * T]), (cfg, b, 'q|k')
            assert torch.equal(vt1[0, :, :T], vt[b, :, :T]), (cfg, b, 'V^T')
    record(f'sample alone {ident(case)}: every sample bit-equal to its rows and its V^T plane of the batch call (cfg 0 and 6)')
