"""First-stage encoder on the GPU: the padded-bottom/right stride-2 convolution alone (op-level ABI), fgdm_vae_encode against the
reference's own AutoencoderKL.encode (tests/golden/vae_enc.npz, vae_enc_ac.npz: tools/make_goldens.py `vae_enc`), the posterior
kernel, the LatentDiffusion mirror, batch independence across the internal chunking, and the image-conditioned sampler entry
points that need an encoded image.  Inputs: synth.image(n, res, seed=res), as the golden generator draws them.

Tolerances: the convolution alone is held to the per-kernel bar of test_gpu_ops.py (1e-3 normwise, LOCAL_TOL blockwise); whole
encodes to check_net (tests/common.py: max(1e-3, 1.09 x the measured autocast floor), capped)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import golden_inputs as gi
from common import GOLD, check_net, gold, relerr, report
from fgdm_amd import _lib, synth
from guarded import LOCAL_TOL, guarded_in, guarded_out, tile_err

pytestmark = pytest.mark.gpu

TOL = 1e-3
SCALE = 0.18215
FS = 'first_stage_model.'


def image(n, res):
    return torch.from_numpy(synth.image(n, res=res, seed=res))


@pytest.fixture(scope='module')
def engine():
    from fgdm_amd.engine import Engine
    e = Engine(gi.SMALL_CFG, vae=True, vae_encoder=True)
    for k, shape in e.param_shapes().items():
        e.load_tensor(k, synth.make_tensor(k, shape))
    e.finalize()
    yield e
    e.close()


@pytest.fixture(scope='module')
def model(engine):
    from fgdm_amd.models import LatentDiffusion
    return LatentDiffusion(engine=engine, use_adapter=False)


@pytest.fixture(scope='module')
def decoder_only():
    """an engine built as before the encoder existed (no weights needed: the calls under test fail before any launch)"""
    from fgdm_amd.engine import Engine
    e = Engine(gi.SMALL_CFG, vae=True)
    yield e
    e.close()


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def h16(x):
    return x.half().float()


def to_rows(x):
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])


def conv_br(x, w, bias):
    """fgdm_op_conv2d with stride = STRIDE2_PAD_BR on fp16-rounded NCHW x (CPU) -> guarded [B Ho Wo, Cout] fp16 output, Ho, Wo"""
    lib = _lib.load()
    B, Cin, H, W = x.shape
    Cout = w.shape[0]
    Ho, Wo = (H - 2) // 2 + 1, (W - 2) // 2 + 1
    xd = guarded_in(x.permute(0, 2, 3, 1).half().contiguous())
    wd, bd = w.contiguous().cuda(), bias.contiguous().cuda()
    out = guarded_out((B * Ho * Wo, Cout), torch.half)
    rc = lib.fgdm_op_conv2d(_p(xd), Cin, None, 0, _p(wd), _p(bd), None, None, B, H, W, Cout, 3, _lib.STRIDE2_PAD_BR, 0, 0, 1.0,
                            _p(out.t), _st())
    assert rc == 0
    torch.cuda.synchronize()
    return out.check(), Ho, Wo


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


BR_CASES = [
    # B, H, W, C: the encoder's first and last Downsample widths, and an odd-sized plane for the boundary arithmetic
    (2, 64, 64, 128, '128->128 on 2x64x64'),
    (1, 16, 16, 512, '512->512 on 1x16x16'),
    (1, 30, 30, 128, '128->128 on 1x30x30 (H/2 = 15: odd output, M tail)'),
    (3, 9, 7, 64, '64->64 on 3x9x7 (odd input: the last tap row / column is in range)'),
]


@pytest.mark.parametrize('case', BR_CASES, ids=[c[-1] for c in BR_CASES])
def test_conv_stride2_pad_bottom_right(case):
    B, H, W, Cc, tag = case
    x = h16(rnd((B, Cc, H, W), 21))
    w = h16(rnd((Cc, Cc, 3, 3), 22, 1.0 / np.sqrt(9 * Cc)))
    bias = rnd((Cc,), 23, 0.1)
    ref = F.conv2d(F.pad(x, (0, 1, 0, 1)), w, bias, stride=2)
    got, Ho, Wo = conv_br(x, w, bias)
    assert (Ho, Wo) == tuple(ref.shape[2:])
    refr = to_rows(ref).cuda()
    e, te = relerr(got, refr), tile_err(got, refr, (32, 32))
    report(f'conv s2 pad-bottom/right {tag} [tile_err {te:.3e}]', e, TOL)
    assert e < TOL, (tag, e)
    assert te < LOCAL_TOL, (tag, 'tile_err', te)
    # the symmetric stride-2 mode is another function of the same operands: the two must not be confused
    sym = F.conv2d(x, w, bias, stride=2, padding=1)
    if sym.shape == ref.shape:
        assert relerr(got, to_rows(sym).cuda()) > 0.1


def test_conv_stride2_pad_bottom_right_every_kernel():
    """The same layer through each kernel the dispatcher may pick for the encoder's Downsamples (forced tile configurations:
    the three 2-stage tiles, then the pipelined 256 x 128 tile with the pipelined and the phase-locked K loop)."""
    lib = _lib.load()
    x = h16(rnd((2, 128, 64, 64), 31))
    w = h16(rnd((128, 128, 3, 3), 32, 1.0 / np.sqrt(9 * 128)))
    bias = rnd((128,), 33, 0.1)
    ref = to_rows(F.conv2d(F.pad(x, (0, 1, 0, 1)), w, bias, stride=2)).cuda()
    outs = []
    try:
        for cfg in (1, 2, 3, 4 + 6 + 32, 4 + 6 + 16):
            assert lib.fgdm_debug_force_igemm_cfg(cfg) == 0
            got, _, _ = conv_br(x, w, bias)
            e = report(f'conv s2 pad-bottom/right 128->128, forced igemm cfg {cfg}', relerr(got, ref), TOL)
            assert e < TOL, cfg
            assert tile_err(got, ref, (32, 32)) < LOCAL_TOL, cfg
            outs.append(got.clone())
    finally:
        lib.fgdm_debug_force_igemm_cfg(0)
    # within a kernel family the tile and the K loop change no bit (the two families round their fp32 sums in different places)
    assert torch.equal(outs[1], outs[0]) and torch.equal(outs[2], outs[0])
    assert torch.equal(outs[4], outs[3])
    print('2-stage vs pipelined kernel:', 'equal bits' if torch.equal(outs[3], outs[0]) else f'rel diff {relerr(outs[3], outs[0]):.3e}')


def test_downsample_vs_reference_golden():
    """encoder.down.0.downsample of the reference on ITS conv_in features of the 64x64 images (vae_enc_down0.npz): conv_in here
    is torch's fp32 conv2d of the same synthetic weights on the CPU, rounded to fp16 as the engine stores activations."""
    want = torch.from_numpy(gold('vae_enc_down0')['down0_y'])
    keys = json.load(open(os.path.join(GOLD, 'vae_encoder_keys.json')))
    t = lambda k: torch.from_numpy(synth.make_tensor(FS + k, keys[FS + k]))
    h = F.conv2d(image(2, 64), t('encoder.conv_in.weight'), t('encoder.conv_in.bias'), padding=1)
    got, Ho, Wo = conv_br(h16(h), h16(t('encoder.down.0.downsample.conv.weight')), t('encoder.down.0.downsample.conv.bias'))
    assert (2, 128, Ho, Wo) == tuple(want.shape)
    refr = to_rows(want).cuda()
    e = report('encoder.down.0.downsample vs reference fp32', relerr(got, refr), TOL)
    assert e < TOL
    assert tile_err(got, refr, (32, 32)) < LOCAL_TOL


@pytest.mark.parametrize('n,res', [(2, 64), (1, 128), (1, 512)])
def test_vae_encode_vs_reference_goldens(engine, n, res):
    g, ga = gold('vae_enc'), gold('vae_enc_ac')
    x = image(n, res)
    if n > 1:
        assert not torch.equal(x[0], x[1])
    moments = engine.vae_encode(x)
    assert tuple(moments.shape) == tuple(g[f'moments_{res}'].shape) == (n, 8, res // 8, res // 8)
    assert moments.dtype == torch.float32 and bool(torch.isfinite(moments).all())
    check_net(f'vae encode {res}x{res} moments', moments.cpu(), g[f'moments_{res}'], ga[f'moments_{res}'])


def _closed_form(moments, noise, scale):
    mean, logvar = torch.chunk(moments, 2, dim=1)
    std = torch.exp(0.5 * torch.clamp(logvar, -30.0, 20.0))
    return scale * (mean + std * noise), scale * (mean.abs() + (std * noise).abs())


def _ulps(got, ref, mag):
    """largest |got - ref| in units of the fp32 spacing at `mag` (elementwise)"""
    spacing = torch.maximum(torch.abs(torch.nextafter(mag, torch.full_like(mag, float('inf'))) - mag),
                            torch.full_like(mag, float(np.finfo(np.float32).tiny)))
    return float(((got.double() - ref.double()).abs() / spacing.double()).max())


def test_posterior_sample_kernel(engine):
    """fgdm_posterior_sample vs the closed form evaluated by torch on the CPU from the SAME moments: within 4 ulp (fp32).

    Both sides are one exp, one multiply, one add and the scale, each rounded separately (the kernel is built without multiply-add
    contraction), so they differ only where the two exp implementations disagree in the last place of std -- which reaches the
    result scaled by |std noise|.  Where mean and std noise cancel, the result is smaller than either term and an ulp of the
    RESULT no longer bounds that error, so the 4 ulp are taken at the magnitude of the result's terms,
    scale (|mean| + |std noise|) >= |z|.  The stricter figure (ulp at |z| itself) is printed, not asserted.

    Measured on an MI355X (moments of the two 64 x 64 images, 512 elements): 2.00 ulp at the terms' magnitude; at |z| itself the
    worst element is 47 ulp off: one where mean and std noise cancel to a few percent of either term.  (With contraction allowed
    the kernel's expf itself lost accuracy, 6 ulp at x = 10: see boundary.hip.)"""
    moments = engine.vae_encode(image(2, 64))
    noise = rnd((2, 4, 8, 8), 41)
    z = engine.posterior_sample(moments, noise.cuda(), SCALE)
    assert tuple(z.shape) == (2, 4, 8, 8)
    want, mag = _closed_form(moments.cpu(), noise, SCALE)
    u = _ulps(z.cpu(), want, mag)
    print(f'posterior sample vs CPU closed form: {u:.2f} ulp at the terms\' magnitude, {_ulps(z.cpu(), want, want.abs()):.2f} ulp at |z|')
    report('posterior sample vs CPU closed form (ulp at the terms\' magnitude / 4)', u / 4, 1.0)
    assert u <= 4.0
    # mode(): bitwise scale * mean
    zm = engine.posterior_sample(moments, None, SCALE)
    assert torch.equal(zm.cpu(), torch.tensor(SCALE, dtype=torch.float32) * moments.cpu()[:, :4])
    assert torch.equal(engine.posterior_sample(moments, None, 1.0), moments[:, :4])
    # the clamp: log-variances of -50 and 40 act as -30 and 20
    syn = rnd((2, 8, 4, 16), 42)
    syn[:, 0] = 0.0          # mean 0 where the variance is clamped from below: z is then std x noise alone
    syn[:, 4] = -50.0
    syn[:, 5] = 40.0
    n2 = rnd((2, 4, 4, 16), 43)
    z2 = engine.posterior_sample(syn.cuda(), n2.cuda(), 1.0).cpu()
    want2, mag2 = _closed_form(syn, n2, 1.0)
    assert bool(torch.isfinite(z2).all())
    assert _ulps(z2, want2, mag2) <= 4.0
    unclamped = syn[:, :4] + torch.exp(0.5 * syn[:, 4:]) * n2
    assert relerr(z2[:, 1], unclamped[:, 1]) > 0.5          # exp(20) x noise would dominate without the clamp
    assert relerr(z2[:, 0], np.exp(-15.0) * n2[:, 0]) < 1e-6                  # exp(0.5 x -30), not exp(0.5 x -50)


def test_encode_first_stage_mirror(engine, model, decoder_only):
    from fgdm_amd.models import DiagonalGaussianDistribution, LatentDiffusion
    g, ga = gold('vae_enc'), gold('vae_enc_ac')
    x = image(2, 64)
    post = model.encode_first_stage(x)
    assert isinstance(post, DiagonalGaussianDistribution) and post.parameters.is_cuda
    assert torch.equal(post.parameters, engine.vae_encode(x))
    torch.manual_seed(7)
    z = model.get_first_stage_encoding(post)
    assert z.is_cuda and tuple(z.shape) == (2, 4, 8, 8)
    check_net('get_first_stage_encoding(encode_first_stage(x)) seed 7', z.cpu(), g['z_sample_64'], ga['z_sample_64'])
    zm = post.mode(model.scale_factor)
    check_net('scale_factor x encode_first_stage(x).mode()', zm.cpu(), g['z_mode_64'], ga['z_mode_64'])
    assert torch.equal(post.mode(), post.mean)
    # a tensor passes through scaled
    t = post.mean.contiguous()
    assert torch.equal(model.get_first_stage_encoding(t), torch.tensor(model.scale_factor, dtype=torch.float32, device=t.device) * t)
    # a first_stage_encode callable overrides the engine
    model.first_stage_encode = lambda img: 'sentinel'
    try:
        assert model.encode_first_stage(x) == 'sentinel'
    finally:
        model.first_stage_encode = None
    model.split_input_params = {'ks_enc': (128, 128)}
    try:
        with pytest.raises(NotImplementedError):
            model.encode_first_stage(x)
    finally:
        del model.split_input_params
    # a model built as before has no encoder, and says which switch adds it
    old = LatentDiffusion(engine=decoder_only, use_adapter=False)
    with pytest.raises(NotImplementedError, match='first_stage_encoder'):
        old.encode_first_stage(x)


def test_vae_encode_is_batch_independent(engine):
    """Image b of a batch is bit-identical to encoding image b alone, also across the internal chunking: at 512 x 512 one
    pass holds six images, so the seventh of a batch of seven is encoded in a second pass."""
    x = image(3, 64)
    all3 = engine.vae_encode(x)
    for b in range(3):
        assert torch.equal(engine.vae_encode(x[b:b + 1])[0], all3[b]), b
    assert torch.equal(engine.vae_encode(x), all3)
    big = torch.from_numpy(synth.image(7, res=512, seed=7)).cuda()
    all7 = engine.vae_encode(big)
    assert bool(torch.isfinite(all7).all())
    for b in (0, 5, 6):
        assert torch.equal(engine.vae_encode(big[b:b + 1])[0], all7[b]), b


def test_round_trip_and_image_conditioned_samplers(engine, model):
    """What the encoder is for: decode(encode(x)), img2img (stochastic_encode + decode) and inpainting (mask=, x0=) from an
    encoded image.  Shape and finiteness only: the sampler arithmetic is pinned in test_gpu_samplers.py."""
    from fgdm_amd import samplers
    x = image(2, 64)
    z0 = model.encode_first_stage(x).mode(model.scale_factor)
    rec = model.decode_first_stage(z0)
    assert tuple(rec.shape) == tuple(x.shape) and bool(torch.isfinite(rec).all())
    c = torch.from_numpy(synth.context(2, seed=5)).cuda()
    uc = torch.from_numpy(synth.context(2, seed=6)).cuda()
    s = samplers.DDIMSampler(model)
    s.make_schedule(ddim_num_steps=4, ddim_eta=0.0, verbose=False)
    torch.manual_seed(3)
    t_enc = 2
    zt = s.stochastic_encode(z0, torch.tensor([t_enc] * 2, device=z0.device))
    out = s.decode(zt, c, t_enc, unconditional_guidance_scale=3.0, unconditional_conditioning=uc)
    assert tuple(out.shape) == tuple(z0.shape) and bool(torch.isfinite(out).all())
    mask = (rnd((2, 1, 8, 8), 9) > 0).float().cuda()
    out2, _ = samplers.DDIMSampler(model).sample(4, 2, (4, 8, 8), conditioning=c, eta=0.0, verbose=False, mask=mask, x0=z0,
                                                 unconditional_guidance_scale=3.0, unconditional_conditioning=uc)
    assert tuple(out2.shape) == tuple(z0.shape) and bool(torch.isfinite(out2).all())


def test_vae_encode_errors(engine, decoder_only):
    for shape, what in (((1, 3, 60, 64), 'multiples of 8'), ((1, 3, 64, 32), 'multiple of 64')):
        with pytest.raises(RuntimeError, match=what):
            engine.vae_encode(torch.zeros(shape))
    with pytest.raises(ValueError):
        engine.vae_encode(torch.zeros(1, 4, 64, 64))
    with pytest.raises(RuntimeError, match='without a first-stage encoder'):
        decoder_only.vae_encode(torch.zeros(1, 3, 64, 64))
    lib = _lib.load()
    x = torch.zeros(2, 8, 8, 64, dtype=torch.half, device='cuda')
    assert lib.fgdm_posterior_sample(None, None, 1.0, _p(x), 1, 4, 64, _st()) == -1
    # the new stride value is a 3x3 mode only
    w = torch.zeros(64, 64, device='cuda')
    assert lib.fgdm_op_conv2d(_p(x), 64, None, 0, _p(w), None, None, None, 2, 8, 8, 64, 1, _lib.STRIDE2_PAD_BR, 0, 0, 1.0, _p(x), _st()) == -1
    # the engine still works after the refused calls
    assert bool(torch.isfinite(engine.vae_encode(image(1, 64))).all())
