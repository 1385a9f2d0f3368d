"""Device noise on the GPU (fgdm_loop_noise_set, fgdm_randn, fgdm_op_rand_bits; include/fgdm.h): the generator against its numpy
restatement (tests/device_noise_ref.py) -- raw words bit for bit, normals against a float64 Box-Muller of the same words -- and the
armed loops against the unarmed loops fed fgdm_randn's planes and against the per-step Python route, bit for bit.

The bar of the normals: the ROCm install documents no ulp errors for logf / sqrtf / sincospif, so the worst error of z against the
float64 value, in ulps of z, was measured once over 2^24 normals (profiles/device_noise_errors.txt); the bar is twice that, the
margin covering argument ranges that sample did not hit.

The reduced synthetic engine (golden_inputs.SMALL_CFG) at 8 x 8 latents, B = 2, at most 6 steps."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import device_noise_ref as ref
import golden_inputs as gi
from fgdm_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0xFEDC_BA98_7654_3210
B, H, W = 2, 8, 8


def _bar_ulp():
    text = open(os.path.join(ROOT, 'profiles', 'device_noise_errors.txt')).read()
    return 2.0 * float(re.search(r'^worst_ulp\s*=\s*([0-9.eE+-]+)', text, re.M).group(1))


def _ulp_error(z32, z64):
    """|z32 - z64| in units of the fp32 spacing at |z64| (exact zeros of the reference must be exact zeros)"""
    ulp = np.spacing(np.abs(z64).astype(np.float32)).astype(np.float64)
    return np.abs(z32.astype(np.float64) - z64) / ulp


@pytest.fixture(scope='module')
def engine():
    from fgdm_amd.engine import Engine
    e = Engine(gi.SMALL_CFG, n_controlnets=0)
    for k, shape in e.param_shapes().items():
        e.load_tensor(k, synth.make_tensor(k, shape))
    e.finalize()
    yield e
    e.close()


def _randn(*a, **k):
    from fgdm_amd import engine as _k
    return _k.randn(*a, device='cuda', **k)


# ------------------------------------------------------------------------------------------------------------ the generator
@pytest.mark.parametrize('base', [(0xFFFFFFFD, 0, 0, 0), (0xFFFFFFFD, 0xFFFFFFFF, 5, 0), (0xFFFFFFFD, 0xFFFFFFFF, 0xFFFFFFFF, 9),
                                  (0xFFFFFFFD, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), (17, 3, 2, 1)])
def test_raw_words_equal_the_restatement(base):
    from fgdm_amd import _lib
    from fgdm_amd.engine import _ptr, _stream
    n = 300                                                     # more than one block of threads, and past the carry at k = 3
    out = torch.full((n, 4), -1, dtype=torch.int32, device='cuda')
    assert _lib.load().fgdm_op_rand_bits(SEED, *base, _ptr(out), n, _stream()) == 0
    got = out.cpu().numpy().view(np.uint32)
    want = np.stack(ref.philox4x32_10(ref.counter_blocks(base, n), ref.seed_key(SEED)), axis=-1)
    assert np.array_equal(got, want)


@pytest.mark.parametrize('per_sample', [4 * 8 * 8, 4 * 12 * 20])
@pytest.mark.parametrize('rows', [1, 3])
def test_normals_against_a_float64_box_muller_of_the_same_words(per_sample, rows):
    bar = _bar_ulp()
    for stream, step, first in ((ref.STREAM_STEP, 0, 0), (ref.STREAM_Q, 7, 5)):
        got = _randn(SEED, stream, step, (rows, per_sample), first_sample=first).cpu().numpy()
        want = ref.randn64(SEED, stream, step, rows, per_sample, first)
        err = _ulp_error(got, want)
        print(f'stream {stream} step {step} rows {rows} per_sample {per_sample}: worst {err.max():.3f} ulp, bar {bar:.3f}')
        assert err.max() <= bar and np.abs(got).max() <= 5.77
    # rows are global samples: a call that starts further in gives the rows of the larger call
    big = _randn(SEED, ref.STREAM_STEP, 3, (rows + 4, per_sample))
    assert torch.equal(_randn(SEED, ref.STREAM_STEP, 3, (rows, per_sample), first_sample=4), big[4:])
    # repeat: every row is sample 0, whatever first_sample
    rep = _randn(SEED, ref.STREAM_STEP, 3, (rows, per_sample), first_sample=2, repeat=True)
    assert all(torch.equal(rep[r], big[0]) for r in range(rows))
    # temperature: one rounding of temperature * z
    t = 0.7
    assert torch.equal(_randn(SEED, ref.STREAM_STEP, 3, (rows, per_sample), temperature=t), big[:rows] * torch.tensor(t, device='cuda'))


def test_mean_variance_and_lag_one_correlation_of_a_million_normals():
    n = 1 << 20
    z = _randn(SEED, ref.STREAM_STEP, 1, (16, n // 16)).cpu().numpy().astype(np.float64).ravel()
    mean, var = z.mean(), z.var()
    lag1 = np.mean((z[:-1] - mean) * (z[1:] - mean)) / var
    print(f'mean {mean:.3e} var {var:.6f} lag1 {lag1:.3e}')
    assert abs(mean) <= 5 / np.sqrt(n) and abs(var - 1) <= 5 * np.sqrt(2 / n) and abs(lag1) <= 5 / np.sqrt(n)


# ------------------------------------------------------------------------------------------------------------ the loops
def _inputs(b=B, seed=900):
    x = torch.from_numpy(synth.latents(b, H, W, seed=seed)).cuda()
    c = torch.from_numpy(synth.context(b, seed=seed + 1)).cuda()
    uc = torch.from_numpy(synth.context(b, seed=seed + 2)).cuda()
    x0 = torch.from_numpy(synth.latents(b, H, W, seed=911)).cuda()
    return x, c, uc, x0


def _mask():
    return (torch.arange(W) < W // 2).float().view(1, 1, 1, W).expand(1, 1, H, W).cuda()


@pytest.fixture()
def recorded(engine, monkeypatch):
    """every sample_ancestral / sample_ddim_ex call of the test, as (name, args, kwargs), run by the real method"""
    calls = type('Calls', (list,), {})()
    for name in ('sample_ancestral', 'sample_ddim_ex'):
        real = getattr(engine, name)
        monkeypatch.setattr(engine, name, (lambda name, real: lambda *a, **k: (calls.append((name, a, k)), real(*a, **k))[1])(name, real))
    calls.real = lambda name: getattr(type(engine), name).__get__(engine)
    return calls


def _planes(stream, S, shape, first_step=0, first_sample=0, repeat=False, temperature=1.):
    return torch.stack([_randn(SEED, stream, first_step + i, shape, first_sample=first_sample, repeat=repeat, temperature=temperature)
                        for i in range(S)])


ANCESTRAL = {
    'mask': dict(mask=True),
    'mask_repeat_temperature': dict(mask=True, repeat_noise=True, temperature=0.7),
}


def _ancestral_kw(name, x0):
    kw = dict(ANCESTRAL[name], timesteps=6)
    if kw.pop('mask', False):
        kw.update(mask=_mask(), x0=x0)
    return kw


def _ldm(engine, loop, seed=SEED):
    from fgdm_amd import models
    return models.LatentDiffusion(gi.SMALL_CFG, engine=engine, use_adapter=False, device_loop=loop, device_noise=seed)


@pytest.mark.parametrize('name', list(ANCESTRAL))
def test_ancestral_armed_loop_fed_planes_and_per_step_route_agree(engine, recorded, name):
    x_T, c, _, x0 = _inputs()
    kw = _ancestral_kw(name, x0)
    armed = _ldm(engine, True).p_sample_loop(c, (B, 4, H, W), x_T=x_T, **kw)
    assert [k[0] for k in recorded] == ['sample_ancestral']
    _, a, k = recorded[0]
    assert k.get('step_noise') is None and k.get('q_noise') is None and k['mask'] is not None
    S, shape = 6, (B, 4, H, W)
    fed = recorded.real('sample_ancestral')(*a, **dict(k, step_noise=_planes(ref.STREAM_STEP, S, shape, repeat=kw.get('repeat_noise', False)),
                                                       q_noise=_planes(ref.STREAM_Q, S, shape)))[0]
    per_step = _ldm(engine, False).p_sample_loop(c, (B, 4, H, W), x_T=x_T, **kw)
    assert len(recorded) == 1                                   # ... which made no loop call
    assert torch.equal(armed, fed) and torch.equal(armed, per_step)
    assert bool(torch.isfinite(armed).all()) and not torch.equal(armed, x_T)
    other = _ldm(engine, True, SEED + 1).p_sample_loop(c, (B, 4, H, W), x_T=x_T, **kw)
    assert not torch.equal(other, armed)


def _sampler(engine, loop, seed=SEED):
    from fgdm_amd import models, samplers
    return samplers.DDIMSampler(models.LatentDiffusion(gi.SMALL_CFG, engine=engine, use_adapter=False), device_loop=loop, device_noise=seed)


def _ddim(sampler, c, uc, x_T, **kw):
    return sampler.sample(5, B, (4, H, W), c, verbose=False, eta=1.0, x_T=x_T, unconditional_guidance_scale=3.0,
                          unconditional_conditioning=uc, log_every_t=2, **kw)


@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('temperature', [1.0, 0.6])
def test_ddim_armed_loop_fed_planes_and_per_step_route_agree(engine, recorded, masked, temperature):
    x_T, c, uc, x0 = _inputs()
    kw = dict(temperature=temperature, **(dict(mask=_mask(), x0=x0) if masked else {}))
    armed, ainter = _ddim(_sampler(engine, True), c, uc, x_T, **kw)
    assert [k[0] for k in recorded] == ['sample_ddim_ex']
    _, a, k = recorded[0]
    assert k.get('step_noise') is None and k.get('q_noise') is None and ('mask' in k) == masked
    S, shape = 5, (B, 4, H, W)
    feed = dict(step_noise=_planes(ref.STREAM_STEP, S, shape, temperature=temperature))
    if masked:
        feed['q_noise'] = _planes(ref.STREAM_Q, S, shape)
    fed = recorded.real('sample_ddim_ex')(*a, **dict(k, **feed))
    per_step, pinter = _ddim(_sampler(engine, False), c, uc, x_T, **kw)
    assert len(recorded) == 1
    assert torch.equal(armed, fed[0]) and torch.equal(armed, per_step) and bool(torch.isfinite(armed).all())
    for key in ('x_inter', 'pred_x0'):
        assert len(ainter[key]) == len(pinter[key]) == 4 and all(torch.equal(u, v) for u, v in zip(ainter[key], pinter[key]))
    assert torch.equal(torch.stack(ainter['x_inter'][1:]), fed[1]) and torch.equal(torch.stack(ainter['pred_x0'][1:]), fed[2])


def test_a_walk_in_two_armed_calls_equals_the_single_call(engine, recorded):
    x_T, c, uc, x0 = _inputs()
    # ancestral: tables and timesteps in walk order
    one = _ldm(engine, True).p_sample_loop(c, (B, 4, H, W), x_T=x_T, **_ancestral_kw('mask', x0))
    _, a, k = recorded[0]
    x, cond, ts, tables = a
    real = recorded.real('sample_ancestral')
    cut = 2
    with engine.loop_noise(SEED):
        mid = real(x, cond, ts[:cut], {n: v[:cut] for n, v in tables.items()}, **k)[0]
    with engine.loop_noise(SEED, first_step=cut):
        two = real(mid, cond, ts[cut:], {n: v[cut:] for n, v in tables.items()}, **k)[0]
    assert torch.equal(one, two)
    with engine.loop_noise(SEED):                                # ... and without first_step the second call repeats the first steps' noise
        assert not torch.equal(real(mid, cond, ts[cut:], {n: v[cut:] for n, v in tables.items()}, **k)[0], one)
    # DDIM: the tables in ddim_timesteps order (the walk runs them backwards), cfg_scales in walk order
    del recorded[:]
    one, _ = _ddim(_sampler(engine, True), c, uc, x_T, mask=_mask(), x0=x0)
    _, a, k = recorded[0]
    x, cond, uncond, scale, ts, alphas, alphas_prev, s1m = a
    S = len(ts)
    real = recorded.real('sample_ddim_ex')

    def part(lo, hi, x_in, first_step):                          # walk steps [lo, hi)
        sl = slice(S - hi, S - lo)
        kk = dict(k, log_steps=(), sigmas=k['sigmas'][sl], cfg_scales=k['cfg_scales'][lo:hi],
                  sqrt_alphas_cumprod_t=k['sqrt_alphas_cumprod_t'][sl], sqrt_one_minus_alphas_cumprod_t=k['sqrt_one_minus_alphas_cumprod_t'][sl])
        with engine.loop_noise(SEED, first_step=first_step):
            return real(x_in, cond, uncond, scale, ts[sl], alphas[sl], alphas_prev[sl], s1m[sl], **kk)[0]
    assert torch.equal(part(cut, S, part(0, cut, x, 0), cut), one)


def test_two_shards_equal_the_rows_of_the_whole_batch(engine):
    x_T, c, uc, x0 = _inputs()
    whole = _ldm(engine, True).p_sample_loop(c, (B, 4, H, W), x_T=x_T, **_ancestral_kw('mask', x0))
    dwhole, _ = _ddim(_sampler(engine, True), c, uc, x_T, mask=_mask(), x0=x0)
    for r in range(B):
        m = _ldm(engine, True)
        m.noise_first_sample = r
        part = m.p_sample_loop(c[r:r + 1], (1, 4, H, W), x_T=x_T[r:r + 1], **dict(_ancestral_kw('mask', x0[r:r + 1])))
        assert torch.equal(part, whole[r:r + 1])
        s = _sampler(engine, True)
        s.noise_first_sample = r
        dpart, _ = s.sample(5, 1, (4, H, W), c[r:r + 1], verbose=False, eta=1.0, x_T=x_T[r:r + 1], unconditional_guidance_scale=3.0,
                            unconditional_conditioning=uc[r:r + 1], log_every_t=2, mask=_mask(), x0=x0[r:r + 1])
        assert torch.equal(dpart, dwhole[r:r + 1])


def test_unarmed_calls_without_noise_are_refused_as_before_and_leave_x_alone(engine, recorded):
    x_T, c, uc, x0 = _inputs()
    _ldm(engine, True).p_sample_loop(c, (B, 4, H, W), x_T=x_T, **_ancestral_kw('mask', x0))
    _ddim(_sampler(engine, True), c, uc, x_T)
    (_, a1, k1), (_, a2, k2) = recorded
    for name, a, k, why in (('sample_ancestral', a1, k1, 'mask needs x0, q_noise'),
                            ('sample_ancestral', a1, dict(k1, mask=None, x0=None), 'a std is not 0 and step_noise is NULL'),
                            ('sample_ddim_ex', a2, k2, 'a sigma is not 0 and step_noise is NULL')):
        out = torch.empty_like(x_T)
        with pytest.raises(RuntimeError, match=why):
            recorded.real(name)(*a, **dict(k, out=out))
        torch.cuda.synchronize()
        assert torch.equal(out, x_T)
    # a plan the library refuses leaves the engine unarmed
    from fgdm_amd import _lib
    p = _lib.FgdmNoisePlan()
    p.struct_size, p.first_step = C.sizeof(p), -1
    assert engine.lib.fgdm_loop_noise_set(engine.h, C.byref(p)) == -1
    p.first_step, p.reserved0 = 0, 1
    assert engine.lib.fgdm_loop_noise_set(engine.h, C.byref(p)) == -1
    p.reserved0, p.struct_size = 0, 24
    assert engine.lib.fgdm_loop_noise_set(engine.h, C.byref(p)) == -1
    with pytest.raises(RuntimeError, match='step_noise is NULL'):
        recorded.real('sample_ddim_ex')(*a2, **k2)
    # ... and the ranges are checked by the armed call
    with engine.loop_noise(SEED, first_step=2 ** 31 - 3):
        with pytest.raises(RuntimeError, match='INT32_MAX'):
            recorded.real('sample_ddim_ex')(*a2, **k2)
