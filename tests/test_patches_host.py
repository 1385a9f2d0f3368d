"""Host side of the patch-wise routes (split_input_params), no GPU: crop geometry and blending tables against the reference's
own (tests/golden/split_input_tables.npz, recorded from LatentDiffusion.get_fold_unfold), argument errors of the stateless C
entries, and the routing of the model mirrors, with a stub engine."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import split_input_inputs as si
from common import gold
from fgdm_amd import _lib, models, patches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('fgdm_unfold', 'fgdm_fold_weighted', 'fgdm_vae_decode_patches', 'fgdm_apply_model_patches')


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from fgdm_amd import build
        build.build(verbose=False)
    return _lib.load()


def _tables(i):
    h, w, ks, stride, uf, tie = si.TABLES[i]
    (kh, kw), st, Ly, Lx = patches.plan(h, w, ks, stride)
    w_pix, w_tie = patches.weights(kh * uf, kw * uf, Ly, Lx, si.split_params(ks, stride, tie))
    return (h * uf, w * uf), (st[0] * uf, st[1] * uf), Lx, w_pix, w_tie


@pytest.mark.parametrize('i', range(len(si.TABLES)))
def test_tables_bit_equal_to_reference(i):
    g = gold('split_input_tables')
    h, w, ks, stride, uf, tie = si.TABLES[i]
    (Ho, Wo), st, Lx, w_pix, w_tie = _tables(i)
    ref = torch.from_numpy(g[f'weighting_{i}'])                        # [1, 1, kh, kw, L]
    assert tuple(ref.shape) == (1, 1, *w_pix.shape, w_tie.numel())
    assert w_pix.dtype == w_tie.dtype == torch.float32
    assert bool((w_tie != 1).any()) == tie
    ours = w_pix[:, :, None] * w_tie[None, None, :]                    # one fp32 rounding, as the fold kernels multiply
    assert torch.equal(ours, ref[0, 0])
    # the folded weighting: the same terms as torch.nn.Fold adds, summed in ascending l (at most 4 terms per cell here: every
    # partial sum is within 2^-24 relative of the exact one, so two orders differ by less than 4 * 2^-23 relative)
    norm = patches.normalization(Ho, Wo, w_pix, w_tie, st, Lx)
    nref = torch.from_numpy(g[f'normalization_{i}'])[0, 0]
    assert norm.shape == nref.shape and bool((nref > 0).all())
    assert float(((norm - nref).abs() / nref).max()) <= 4 * 2.0 ** -23


def test_plan_counts_clamps_and_refuses():
    assert patches.plan(24, 40, (16, 16), (8, 8)) == ((16, 16), (8, 8), 2, 4)
    assert patches.plan(24, 40, (16, 8), (8, 8)) == ((16, 8), (8, 8), 2, 5)
    assert patches.plan(24, 40, (12, 8), (4, 8)) == ((12, 8), (4, 8), 4, 5)
    # decode_first_stage's clamping (ddpm.py:847-853): kernel and stride reduced to the grid, per axis
    assert patches.plan(16, 24, (128, 128), (64, 64)) == ((16, 24), (16, 24), 1, 1)
    assert patches.plan(16, 24, (128, 8), (64, 4)) == ((16, 8), (16, 4), 1, 5)
    with pytest.raises(ValueError):      # apply_model does not clamp: a crop larger than the grid is refused
        patches.plan(16, 24, (128, 128), (64, 64), clamp=False)
    for h, w, ks, st in ((24, 40, (16, 16), (8, 7)),      # (w - kw) % sw != 0: the last columns are in no crop
                         (25, 40, (16, 16), (8, 8)),      # (h - kh) % sh != 0
                         (24, 40, (8, 8), (16, 8)),       # stride > ks: gaps between the crops
                         (24, 40, (1, 8), (1, 8)),        # ks < 2: delta_border divides by ks - 1
                         (24, 40, (8, 1), (8, 1)),
                         (24, 40, (8, 8), (0, 8))):
        with pytest.raises(ValueError):
            patches.plan(h, w, ks, st)


def test_delta_border_is_the_reference_formula():
    d = patches.delta_border(5, 9)
    assert d.dtype == torch.float32 and tuple(d.shape) == (5, 9)
    assert float(d[0].max()) == 0 and float(d[-1].max()) == 0 and float(d[:, 0].max()) == 0 and float(d[:, -1].max()) == 0
    assert float(d[2, 4]) == 0.5 and float(d[1, 4]) == 0.25 and float(d[2, 1]) == 0.125


def test_decode_needs_a_square_crop():
    sp = si.split_params((16, 8), (8, 8))
    with pytest.raises(ValueError, match='square'):
        patches.decode_geometry(24, 40, sp)
    assert patches.decode_geometry(16, 24, si.split_params(si.VAE_KS, si.VAE_STRIDE)) == ((8, 8), (4, 4), 3, 5, 8)


def test_abi_declares_the_patch_entries(lib):
    hdr = open(os.path.join(ROOT, 'include', 'fgdm.h')).read()
    declared = set(re.findall(r'\b(fgdm_[a-z0-9_]+)\s*\(', hdr))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name


def test_stateless_entries_refuse_bad_arguments(lib):
    """FGDM_ERR_ARG before any launch (so without a GPU too): the pointers below are never dereferenced."""
    p, null = C.c_void_p(1 << 20), None
    unfold = lambda x, o, H, W, kh, kw, sh, sw, l0, n: lib.fgdm_unfold(x, 2, 4, H, W, kh, kw, sh, sw, l0, n, o, null)
    assert unfold(null, p, 24, 40, 16, 16, 8, 8, 0, 8) == -1 and unfold(p, null, 24, 40, 16, 16, 8, 8, 0, 8) == -1
    assert unfold(p, p, 24, 40, 32, 16, 8, 8, 0, 1) == -1        # crop larger than the grid
    assert unfold(p, p, 24, 40, 16, 16, 0, 8, 0, 1) == -1        # stride 0
    assert unfold(p, p, 24, 40, 16, 16, 8, 8, 7, 2) == -1        # crops [7, 9) of 8
    assert unfold(p, p, 24, 40, 16, 16, 8, 8, -1, 2) == -1 and unfold(p, p, 24, 40, 16, 16, 8, 8, 0, 0) == -1
    fold = lambda o, wp, wt, y, Ho, Wo, kh, kw, sh, sw, cpp=0: lib.fgdm_fold_weighted(o, wp, wt, 2, 4, Ho, Wo, kh, kw, sh, sw, cpp, y, null)
    for args in ((null, p, p, p), (p, null, p, p), (p, p, null, p), (p, p, p, null)):
        assert fold(*args, 24, 40, 16, 16, 8, 8) == -1
    assert fold(p, p, p, p, 24, 40, 16, 16, 8, 7) == -1          # uncovered columns
    assert fold(p, p, p, p, 25, 40, 16, 16, 8, 8) == -1          # uncovered rows
    assert fold(p, p, p, p, 24, 40, 8, 8, 16, 8) == -1           # stride > ks
    assert fold(p, p, p, p, 24, 40, 16, 16, 8, 8, -1) == -1      # negative pass size
    # the engine entries without an engine
    assert lib.fgdm_vae_decode_patches(null, p, 1, 16, 24, 1.0, 8, 8, 4, 4, 8, p, p, 0, p, null) == -1
    assert lib.fgdm_apply_model_patches(null, p, p, null, p, 1, 24, 32, 16, 16, 8, 8, p, p, 0, 0, p, null) == -1


# ---------------------------------------------------------------------------------------------------------------- routing
class StubEngine:
    """Records the engine methods the model mirrors call (no GPU, no library)."""
    has_vae, has_vae_encoder, has_clip, n_controlnets = True, False, False, 0
    device = torch.device('cpu')

    def __init__(self):
        self.calls = []

    def apply_model(self, x, t, ctx, control_scales=None, flags=0, pcond=None, out=None):
        self.calls.append(('apply_model', tuple(x.shape), tuple(ctx.shape), flags, pcond))
        return torch.zeros_like(x)

    def vae_decode(self, z, scale=1.0):
        self.calls.append(('vae_decode', tuple(z.shape), scale))
        return torch.zeros(z.shape[0], 3, 8 * z.shape[2], 8 * z.shape[3])

    def apply_model_patches(self, x, t, ctx, ks, stride, w_pix, w_tie, max_crops_per_pass=0, flags=0):
        self.calls.append(('apply_model_patches', tuple(x.shape), tuple(ctx.shape), tuple(ks), tuple(stride), w_pix, w_tie,
                           max_crops_per_pass, flags))
        return torch.zeros_like(x)

    def vae_decode_patches(self, z, scale, ks, stride, f, w_pix, w_tie, max_crops_per_pass=0):
        self.calls.append(('vae_decode_patches', tuple(z.shape), scale, tuple(ks), tuple(stride), f, w_pix, w_tie,
                           max_crops_per_pass))
        return torch.zeros(z.shape[0], 3, f * z.shape[2], f * z.shape[3])


def _model():
    return models.LatentDiffusion(engine=StubEngine(), use_adapter=False)


def test_without_the_attribute_the_plain_engine_methods_run():
    m = _model()
    x, t, c = torch.zeros(2, 4, 24, 32), torch.tensor([5, 5]), torch.zeros(2, 77, 768)
    m.apply_model(x, t, c)
    m.apply_model(x, t, [c], use_original=True, cfg_pairs=True)
    m.decode_first_stage(x)
    assert m.engine.calls == [('apply_model', (2, 4, 24, 32), (2, 77, 768), _lib.FLAG_NO_CONTROL, None),
                              ('apply_model', (2, 4, 24, 32), (2, 77, 768),
                               _lib.FLAG_NO_CONTROL | _lib.FLAG_USE_ORIGINAL | _lib.FLAG_CFG_PAIRS, None),
                              ('vae_decode', (2, 4, 24, 32), 1. / m.scale_factor)]
    # patch_distributed_vq false: the decode stays plain although the attribute exists (ddpm.py:879-883)
    m.split_input_params = dict(si.split_params((8, 8), (4, 4)), patch_distributed_vq=False)
    m.decode_first_stage(x)
    assert m.engine.calls[-1] == ('vae_decode', (2, 4, 24, 32), 1. / m.scale_factor)


def test_with_the_attribute_the_patch_methods_run():
    m = _model()
    m.split_input_params = si.split_params((16, 16), (8, 8))
    x, t, c = torch.zeros(2, 4, 24, 32), torch.tensor([5, 5]), torch.zeros(2, 77, 768)
    m.apply_model(x, t, c, use_original=True, cfg_pairs=True, pcond=x)      # kwargs are not forwarded to the crops (ddpm.py:1119)
    name, xs, cs, ks, st, w_pix, w_tie, mc, flags = m.engine.calls[-1]
    assert (name, xs, cs, ks, st, mc, flags) == ('apply_model_patches', (2, 4, 24, 32), (2, 77, 768), (16, 16), (8, 8), 0, 0)
    want = patches.weights(16, 16, 2, 3, m.split_input_params)
    assert torch.equal(w_pix, want[0]) and torch.equal(w_tie, want[1])
    m.apply_model(x, t, c)
    assert m.engine.calls[-1][5] is w_pix          # the tables are computed once per geometry
    m.max_crops_per_pass = 2
    m.decode_first_stage(torch.zeros(1, 4, 16, 24))      # uf = vqf = 8: tables at image resolution
    name, zs, scale, ks, st, f, w_pix, w_tie, mc = m.engine.calls[-1]
    assert (name, zs, scale, ks, st, f, mc) == ('vae_decode_patches', (1, 4, 16, 24), 1. / m.scale_factor, (16, 16), (8, 8), 8, 2)
    assert tuple(w_pix.shape) == (128, 128) and tuple(w_tie.shape) == (2,)
    with pytest.raises(AssertionError):
        m.apply_model(x, t, c, return_ids=True)
    with pytest.raises(AssertionError):
        m.apply_model(x, t, {'c_crossattn': [c], 'c_concat': [x]})
    with pytest.raises(ValueError):
        m.apply_model(torch.zeros(2, 4, 24, 30), t, c)        # (30 - 16) % 8 != 0
    for key in patches.SPATIAL_COND_KEYS:
        m.cond_stage_key = key
        with pytest.raises(NotImplementedError):
            m.apply_model(x, t, c)
    m.split_input_params = si.split_params((16, 8), (8, 8))
    with pytest.raises(ValueError, match='square'):
        m.decode_first_stage(torch.zeros(1, 4, 24, 40))
    with pytest.raises(NotImplementedError, match='DiagonalGaussianDistribution'):
        m.encode_first_stage(torch.zeros(1, 3, 64, 64))
