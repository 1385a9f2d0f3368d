"""Patch-wise routes (split_input_params) on the GPU: the unfold / weighted-fold kernels against torch.nn.Unfold and a float64
evaluation of fold(o * w) / fold(w); LatentDiffusion.apply_model and decode_first_stage with the attribute set against the
reference's own patch-wise results (tests/golden/split_input_*.npz, made by tools/make_goldens.py from ddpm.py:841-878 and
:1046-1128), under the unchanged whole-network rule of tests/common.py: check_net."""
import numpy as np
import pytest
import torch

import golden_inputs as gi
import split_input_inputs as si
from common import check_net, gold, report
from fgdm_amd import _lib, engine as eng, models, patches, samplers, synth
from guarded import guarded_in, guarded_out

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24


# ---------------------------------------------------------------------------------------------------------------- unfold
def _unfold_ref(x, ks, stride):
    B, C = x.shape[:2]
    cols = torch.nn.Unfold(kernel_size=ks, stride=stride)(x)                    # [B, C kh kw, L]
    return cols.view(B, C, ks[0], ks[1], -1).permute(4, 0, 1, 2, 3).contiguous()   # [L, B, C, kh, kw]


@pytest.mark.parametrize('ks,stride,l0,n', [((16, 16), (8, 8), 0, None), ((16, 8), (8, 8), 0, None), ((8, 8), (8, 8), 0, None),
                                            ((24, 40), (24, 40), 0, None), ((16, 16), (8, 8), 3, 2),
                                            ((6, 5), (3, 7), 0, None)])
def test_unfold_is_torch_unfold(ks, stride, l0, n):
    """bit-equal to torch.nn.Unfold viewed as [L,B,C,kh,kw]; the last case has odd widths (the scalar kernel)"""
    x = torch.from_numpy(synth.latents(2, 24, 40, seed=2300))
    ref = _unfold_ref(x, ks, stride)
    n_ = ref.shape[0] - l0 if n is None else n
    out = guarded_out((n_, 2, 4, ks[0], ks[1]), torch.float32)
    eng.unfold(guarded_in(x), ks, stride, l0, n, out=out.t)
    torch.cuda.synchronize()
    assert torch.equal(out.check().cpu(), ref[l0:l0 + n_])


# ---------------------------------------------------------------------------------------------------------------- fold
def _fold_ref(o, w_pix, w_tie, size, stride):
    """float64 fold(o * w) / fold(w) from the fp32 inputs, with the per-pixel bound of the fp32 evaluation: n products w_i o_i
    of a rounded weight (2 roundings each), n - 1 additions, the same for the divisor, one division ->
    |got - ref| <= 2 (n + 2) 2^-24 sum|w_i o_i| / sum w_i"""
    L, B, C, kh, kw = o.shape
    Ho, Wo = size
    Lx = (Wo - kw) // stride[1] + 1
    num = torch.zeros(B, C, Ho, Wo, dtype=torch.float64)
    mag = torch.zeros_like(num)
    den = torch.zeros(Ho, Wo, dtype=torch.float64)
    cnt = torch.zeros(Ho, Wo, dtype=torch.float64)
    for l in range(L):
        y0, x0 = (l // Lx) * stride[0], (l % Lx) * stride[1]
        w = w_pix.double() * w_tie[l].double()
        num[:, :, y0:y0 + kh, x0:x0 + kw] += w * o[l].double()
        mag[:, :, y0:y0 + kh, x0:x0 + kw] += w * o[l].double().abs()
        den[y0:y0 + kh, x0:x0 + kw] += w
        cnt[y0:y0 + kh, x0:x0 + kw] += 1
    assert bool((cnt >= 1).all())
    return num / den, 2 * (cnt + 2) * EPS * mag / den, int(cnt.max())


@pytest.mark.parametrize('h,w,ks,stride,tie,cover', [(24, 40, (16, 16), (8, 8), False, 4), (24, 40, (16, 8), (8, 8), False, 2),
                                                     (24, 40, (16, 16), (8, 8), True, 4), (24, 40, (12, 8), (4, 8), False, 3),
                                                     (128, 192, (64, 64), (32, 32), False, 4), (21, 26, (6, 5), (3, 3), True, 4)])
def test_fold_weighted_within_derived_bound(h, w, ks, stride, tie, cover):
    (kh, kw), st, Ly, Lx = patches.plan(h, w, ks, stride)
    L = Ly * Lx
    w_pix, w_tie = patches.weights(kh, kw, Ly, Lx, si.split_params(ks, stride, tie))
    o = torch.from_numpy(synth._rng('fold.o', 2400 + h).standard_normal((L, 2, 3, kh, kw), dtype=np.float32))
    ref, bound, nmax = _fold_ref(o, w_pix, w_tie, (h, w), st)
    assert nmax == cover
    od, outs = guarded_in(o), []
    for cpp in (0, 1, 2):
        out = guarded_out((2, 3, h, w), torch.float32)
        eng.fold_weighted(od, w_pix, w_tie, (h, w), st, crops_per_pass=cpp, out=out.t)
        torch.cuda.synchronize()
        outs.append(out.check().cpu())
    err = (outs[0].double() - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f'fold {h}x{w} ks {ks} stride {stride} tie {tie}: max |err| {float(err.max()):.3e}, worst err / bound {worst:.3f}')
    assert bool((err <= bound).all()), worst
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])      # passes of L, 1 and 2 crops: the same bits


# ---------------------------------------------------------------------------------------------------------------- UNet
@pytest.fixture(scope='module')
def unet_model():
    e = eng.Engine(gi.SMALL_CFG)            # the reduced UNet of small_nets.npz (weights hashed with the generator's 'small.' prefix)
    for k, shape in e.param_shapes().items():
        e.load_tensor(k, synth.make_tensor(k.replace('model.diffusion_model.', 'small.'), shape))
    e.finalize()
    m = models.LatentDiffusion(engine=e, use_adapter=False)
    m.split_input_params = si.split_params(si.UNET_KS, si.UNET_STRIDE)
    yield m
    e.close()


def test_apply_model_patches_vs_reference(unet_model):
    g, ga = gold('split_input_unet'), gold('split_input_unet_ac')
    x, ctx, t = si.unet_x(), si.unet_ctx().cuda(), torch.tensor(si.T)
    eps = unet_model.apply_model(x, t, ctx)
    assert tuple(eps.shape) == tuple(g['eps'].shape)
    check_net('patch-wise apply_model 24x32, 16x16 crops / stride 8', eps.cpu(), g['eps'], ga['eps'])
    # the folded result differs from the whole-latent evaluation: the branch really ran
    sp = unet_model.__dict__.pop('split_input_params')
    try:
        whole = unet_model.apply_model(x, t, ctx)
    finally:
        unet_model.split_input_params = sp
    assert not torch.equal(whole, eps)
    # FGDM_FLAG_CFG_PAIRS requested (by the sampler's keyword, and straight at the engine): the same bits
    assert torch.equal(unet_model.apply_model(x, t, ctx, cfg_pairs=True), eps)
    (kh, kw), st, Ly, Lx = patches.plan(24, 32, si.UNET_KS, si.UNET_STRIDE)
    w_pix, w_tie = patches.weights(kh, kw, Ly, Lx, sp)
    e = unet_model.engine
    assert torch.equal(e.apply_model_patches(x, t, ctx, (kh, kw), st, w_pix, w_tie, flags=_lib.FLAG_CFG_PAIRS), eps)
    # passes of 1 and 4 crops (the last pass shorter): the per-crop results do not depend on the batch they ran in
    for mc in (1, 4):
        assert torch.equal(e.apply_model_patches(x, t, ctx, (kh, kw), st, w_pix, w_tie, max_crops_per_pass=mc), eps), mc


def test_samplers_reach_the_patch_branch(unet_model):
    """3 DDIM steps.  The uniform DDIM spacing needs a step count that divides the schedule (3 on 1000 steps selects timestep
    1000, out of range in the reference too), so the mirror here carries a 900-step schedule over the same engine: t = 1, 301, 601."""
    m = models.LatentDiffusion(engine=unet_model.engine, use_adapter=False, timesteps=900)
    x_T = si.unet_x().cuda()
    c, uc = si.unet_ctx().cuda(), torch.from_numpy(synth.context(2, seed=2102)).cuda()
    run = lambda: samplers.DDIMSampler(m).sample(3, 2, (4, 24, 32), conditioning=c, x_T=x_T, eta=0.0, verbose=False,
                                                 unconditional_guidance_scale=3.0, unconditional_conditioning=uc)[0]
    plain = run()
    m.split_input_params = unet_model.split_input_params
    with_patches = run()
    assert bool(torch.isfinite(with_patches).all()) and tuple(with_patches.shape) == (2, 4, 24, 32)
    assert not torch.equal(with_patches, plain)


# ---------------------------------------------------------------------------------------------------------------- decode
def _vae_engine():
    e = eng.Engine(gi.SMALL_CFG, vae=True)
    for k, shape in e.param_shapes().items():
        e.load_tensor(k, synth.make_tensor(k, shape))
    e.finalize()
    return e


@pytest.fixture(scope='module')
def vae_model():
    e = _vae_engine()
    m = models.LatentDiffusion(engine=e, use_adapter=False)
    m.split_input_params = si.split_params(si.VAE_KS, si.VAE_STRIDE)
    yield m
    e.close()


def test_decode_patches_vs_reference(vae_model):
    g, ga = gold('split_input_vae'), gold('split_input_vae_ac')
    img = vae_model.decode_first_stage(si.vae_z())
    assert tuple(img.shape) == tuple(g['img'].shape) == (1, 3, 128, 192)
    check_net('patch-wise decode_first_stage 16x24, 8x8 crops / stride 4', img.cpu(), g['img'], ga['img'])
    # one crop per pass and the decoder's own rule (here: all 15 crops as one batch) give the same bits: the plain decoder
    # decodes image b of a batch as it decodes it alone (tests/test_gpu_vae.py::test_vae_decode_is_batch_independent)
    vae_model.max_crops_per_pass = 1
    try:
        assert torch.equal(vae_model.decode_first_stage(si.vae_z()), img)
    finally:
        del vae_model.max_crops_per_pass


def test_decode_workspace_follows_the_pass_not_the_image():
    e = _vae_engine()
    try:
        sp = si.split_params(si.VAE_KS, si.VAE_STRIDE)
        peaks = []
        for w in (24, 40):
            (kh, kw), st, Ly, Lx, f = patches.decode_geometry(16, w, sp)
            w_pix, w_tie = patches.weights(kh * f, kw * f, Ly, Lx, sp)
            img = e.vae_decode_patches(si.vae_z(w), 1 / 0.18215, (kh, kw), st, f, w_pix, w_tie, max_crops_per_pass=2)
            assert tuple(img.shape) == (1, 3, 128, 8 * w) and bool(torch.isfinite(img).all())
            peaks.append(e.workspace_stats()['peak_bytes'])
        assert peaks[0] == peaks[1] > 0, peaks
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------------------- errors
def _refused(fn, text):
    with pytest.raises(RuntimeError) as ei:
        fn()
    assert 'failed (-1)' in str(ei.value) and text in str(ei.value), str(ei.value)


def test_argument_errors(vae_model, unet_model):
    x, ctx, t = si.unet_x(), si.unet_ctx().cuda(), torch.tensor(si.T)
    one = torch.ones(16, 16), torch.ones(6)
    cn = eng.Engine(gi.SMALL_CFG, n_controlnets=1)
    try:
        _refused(lambda: cn.apply_model_patches(x, t, ctx, (16, 16), (8, 8), *one), 'no patch branch')
    finally:
        cn.close()
    e = unet_model.engine
    _refused(lambda: e.apply_model_patches(x[..., :30].contiguous(), t, ctx, (16, 16), (8, 8), *one), 'do not cover')
    _refused(lambda: e.apply_model_patches(x, t, ctx, (8, 8), (16, 8), torch.ones(8, 8), torch.ones(8)), 'do not cover')
    v, z = vae_model.engine, si.vae_z()
    w64 = torch.ones(64, 64), torch.ones(15)
    _refused(lambda: v.vae_decode_patches(z, 1.0, (8, 8), (4, 4), 4, torch.ones(32, 32), torch.ones(15)), 'must equal')
    _refused(lambda: v.vae_decode_patches(z, 1.0, (4, 4), (4, 4), 8, torch.ones(32, 32), torch.ones(24)), 'multiple of 64')
    _refused(lambda: v.vae_decode_patches(z, 1.0, (8, 8), (4, 5), 8, *w64), 'do not cover')
    _refused(lambda: v.vae_decode_patches(z, 1.0, (8, 8), (16, 16), 8, *w64), 'do not cover')
