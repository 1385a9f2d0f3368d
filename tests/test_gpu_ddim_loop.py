"""The device DDIM loop (fgdm_sample_ddim_ex, k_ddim_loop_step) on the GPU.

The yardstick is torch.equal: DDIMSampler / ControlDDIMSampler(model, device_loop=True) against the same sampler's per-step route
on the same engine from the same generator state.  Both routes run the same networks and the same arithmetic, rounding for
rounding (the step kernel reproduces fgdm_ddim_step, then fgdm_axpby, then fgdm_mask_blend), so there is no tolerance.
The reduced synthetic engine (golden_inputs.SMALL_CFG) at 8 x 8 latents, S = 4 or 5 (1000 // S must divide
evenly: make_schedule's uniform timesteps reach 1000 otherwise, as the reference's do).  Every run of the loop writes its state and its
intermediates into guarded buffers (tests/guarded.py): a store outside [n_log, B,4,H,W] or the state damages a guard."""
import ctypes as C

import numpy as np
import pytest
import torch

import golden_inputs as gi
from fgdm_amd import synth
from guarded import guarded_in, guarded_out

pytestmark = pytest.mark.gpu

ERR_ARG = -1


@pytest.fixture(scope='module')
def engine():
    from fgdm_amd.engine import Engine
    e = Engine(gi.SMALL_CFG, n_controlnets=1)
    for k, shape in e.param_shapes().items():
        e.load_tensor(k, synth.make_tensor(k, shape))
    e.finalize()
    yield e
    e.close()


@pytest.fixture()
def guard(engine, monkeypatch):
    """every sample_ddim_ex of the test runs on guarded buffers, checked when the call returns"""
    real = engine.sample_ddim_ex
    runs = []

    def guarded(x_T, *a, **k):
        n_log = len(k.get('log_steps', ()))
        gx = guarded_out(tuple(x_T.shape), torch.float32)
        gi_, gp = (guarded_out((n_log, *x_T.shape), torch.float32) for _ in range(2)) if n_log else (None, None)
        out = real(x_T, *a, **k, out=gx.t, x_inter_out=gi_ and gi_.t, pred_x0_out=gp and gp.t)
        torch.cuda.synchronize()
        for g in (gx, gi_, gp):
            if g is not None:
                g.check()
        runs.append(n_log)
        return out
    monkeypatch.setattr(engine, 'sample_ddim_ex', guarded)
    return runs


def _ldm(engine):
    from fgdm_amd import models
    return models.LatentDiffusion(gi.SMALL_CFG, engine=engine, use_adapter=False)


def _cldm(engine):
    from fgdm_amd import models
    m = models.ControlLDM(gi.SMALL_CFG, engine=engine, n_controlnets=1)
    m.control_scales = [0.9] * 13
    return m


def _inputs(B=2, H=8, W=8, seed=700):
    x = torch.from_numpy(synth.latents(B, H, W, seed=seed)).cuda()
    c = torch.from_numpy(synth.context(B, seed=seed + 1)).cuda()
    uc = torch.from_numpy(synth.context(B, seed=seed + 2)).cuda()
    return x, c, uc


def _both(make, run, guard, loops=1, seed=1234):
    """run(sampler) on the per-step route, then on the device loop from the same generator state; the results, bit for bit"""
    outs = []
    for loop in (False, True):
        torch.manual_seed(seed)
        outs.append(run(make(loop)))
    assert len(guard) == loops, 'the device loop did not take this sampling over'
    return outs


def _same(a, b):
    (xa, ia), (xb, ib) = a, b
    assert torch.equal(xa, xb) and bool(torch.isfinite(xa).all())
    for key in ('x_inter', 'pred_x0'):
        assert len(ia[key]) == len(ib[key]), key
        for j, (u, v) in enumerate(zip(ia[key], ib[key])):
            assert torch.equal(u, v), (key, j)
    return xa


def _half_mask(H, W):
    return (torch.arange(W) < W // 2).float().view(1, 1, 1, W).expand(1, 1, H, W).cuda()


# cases through DDIMSampler.sample on the LatentDiffusion mirror; (B, H, W), S, then sample()'s keywords
CASES = {
    'eta0_cfg': ((2, 8, 8), 5, dict(scale=7.5)),
    'cfg_off_no_uncond': ((2, 8, 8), 4, dict(scale=7.5, uc=False)),
    'cfg_off_scale_1': ((2, 8, 8), 4, dict(scale=1.0)),
    'eta_temperature': ((2, 8, 8), 5, dict(scale=7.5, eta=0.7, temperature=0.8)),
    'inpaint_eta0': ((2, 8, 8), 4, dict(scale=5.0, mask='half')),
    'inpaint_eta05': ((2, 8, 8), 4, dict(scale=5.0, mask='half', eta=0.5)),
    'inpaint_zeros': ((2, 8, 8), 4, dict(scale=5.0, mask='zeros', eta=0.5)),
    'inpaint_ones': ((2, 8, 8), 4, dict(scale=5.0, mask='ones', eta=0.5)),
    'log_every_step': ((2, 8, 8), 5, dict(scale=7.5, eta=0.3, log_every_t=1)),
    'log_last_only': ((2, 8, 8), 5, dict(scale=7.5, log_every_t=1000)),
    'batch_1': ((1, 8, 8), 4, dict(scale=7.5, eta=0.5, mask='half')),
    'batch_3_8x16': ((3, 8, 16), 4, dict(scale=7.5, eta=0.5, mask='half', log_every_t=1)),
}


@pytest.mark.parametrize('name', list(CASES))
def test_device_loop_equals_per_step_route(engine, guard, name):
    from fgdm_amd import samplers
    (B, H, W), S, kw = CASES[name]
    kw = dict(kw)
    x_T, c, uc = _inputs(B, H, W)
    scale, use_uc, mask = kw.pop('scale'), kw.pop('uc', True), kw.pop('mask', None)
    if mask:
        kw['x0'] = torch.from_numpy(synth.latents(B, H, W, seed=711)).cuda()
        kw['mask'] = {'half': _half_mask(H, W), 'zeros': torch.zeros(1, 1, H, W).cuda(), 'ones': torch.ones(B, 1, H, W).cuda()}[mask]
    m = _ldm(engine)
    smp = {}

    def run(s):
        smp[s.device_loop] = s
        return s.sample(S, B, (4, H, W), c, verbose=False, x_T=x_T, unconditional_guidance_scale=scale,
                        unconditional_conditioning=uc if use_uc else None, **kw)
    a, b = _both(lambda loop: samplers.DDIMSampler(m, device_loop=loop), run, guard)
    out = _same(a, b)
    n_logged = len(b[1]['x_inter']) - 1
    assert guard == [n_logged] and n_logged == {'log_every_step': S, 'batch_3_8x16': S}.get(name, 2)
    assert not torch.equal(out, x_T)
    if mask == 'ones':          # the last blend (in front of the last step) replaced everything: the result does not depend on x_T
        torch.manual_seed(1234)
        other = smp[True].sample(S, B, (4, H, W), c, verbose=False, x_T=x_T * 0.5, unconditional_guidance_scale=scale,
                                 unconditional_conditioning=uc, **kw)[0]
        assert torch.equal(other, out)
    if name == 'eta0_cfg':      # ... and the plain entry, which is the same loop with every option absent
        from fgdm_amd import _lib
        s = smp[True]
        plain = engine.sample_ddim(x_T, c, uc, scale, s.ddim_timesteps, s.ddim_alphas, s.ddim_alphas_prev,
                                   s.ddim_sqrt_one_minus_alphas, flags=_lib.FLAG_NO_CONTROL)
        assert torch.equal(plain, out)


def test_decode_from_t_start(engine, guard):
    from fgdm_amd import samplers
    x, c, uc = _inputs()
    m = _ldm(engine)

    def run(s):
        s.make_schedule(5, ddim_eta=0.4, verbose=False)
        return s.decode(x, c, 3, unconditional_guidance_scale=6.0, unconditional_conditioning=uc)
    a, b = _both(lambda loop: samplers.DDIMSampler(m, device_loop=loop), run, guard)
    assert torch.equal(a, b) and not torch.equal(a, x) and guard == [0]


def test_original_steps_through_ddim_sampling(engine, guard):
    from fgdm_amd import samplers
    x_T, c, uc = _inputs()
    m = _ldm(engine)

    def run(s):
        s.make_schedule(5, ddim_eta=0.5, verbose=False)
        return s.ddim_sampling(c, (2, 4, 8, 8), x_T=x_T, ddim_use_original_steps=True, timesteps=4, log_every_t=2,
                               unconditional_guidance_scale=7.5, unconditional_conditioning=uc)
    a, b = _both(lambda loop: samplers.DDIMSampler(m, device_loop=loop), run, guard)
    _same(a, b)
    assert guard == [3]          # index 3, 2 and 0 of the four steps


@pytest.mark.parametrize('ucg', [None, [9.0, 7.5, 4.0, 2.5]])
def test_control_sampler_with_hints_and_ucg_schedule(engine, guard, ucg):
    from fgdm_amd import samplers
    x_T, c, uc = _inputs()
    hint = torch.from_numpy(synth.hint(2, res=64, seed=703)).cuda()
    cond, ucond = {'c_concat': [hint], 'c_crossattn': [c]}, {'c_concat': [hint], 'c_crossattn': [uc]}
    m = _cldm(engine)
    run = lambda s: s.sample(4, 2, (4, 8, 8), cond, verbose=False, x_T=x_T, eta=0.3, unconditional_guidance_scale=9.0,
                             unconditional_conditioning=ucond, ucg_schedule=ucg, log_every_t=2)
    a, b = _both(lambda loop: samplers.ControlDDIMSampler(m, device_loop=loop), run, guard)
    out = _same(a, b)
    if ucg is not None:          # the per-step scales matter
        torch.manual_seed(1234)
        flat = samplers.ControlDDIMSampler(m, device_loop=True).sample(
            4, 2, (4, 8, 8), cond, verbose=False, x_T=x_T, eta=0.3, unconditional_guidance_scale=9.0,
            unconditional_conditioning=ucond, log_every_t=2)[0]
        assert not torch.equal(flat, out)
    # ... and so does the hint
    torch.manual_seed(1234)
    other = {'c_concat': [hint.flip(-1).contiguous()], 'c_crossattn': [c]}
    moved = samplers.ControlDDIMSampler(m, device_loop=True).sample(
        4, 2, (4, 8, 8), other, verbose=False, x_T=x_T, eta=0.3, unconditional_guidance_scale=9.0,
        unconditional_conditioning={'c_concat': other['c_concat'], 'c_crossattn': [uc]}, ucg_schedule=ucg, log_every_t=2)[0]
    assert not torch.equal(moved, out)


# ------------------------------------------------------------------------------------------------------------ argument errors
def _params(engine, x, c, uc, **over):
    S = 4
    from fgdm_amd import _lib
    from oracle import schedule
    tab = schedule.ddim_tables(schedule.register_schedule()['alphas_cumprod'], S, 0.0)
    keep = []

    def arr(v, ty=C.c_float):
        keep.append((ty * len(v))(*[ty(x).value for x in v]))
        return C.cast(keep[-1], C.c_void_p)
    p = _lib.FgdmDdimParams()
    p.struct_size = C.sizeof(p)
    p.x, p.cond, p.uncond = x.data_ptr(), c.data_ptr(), uc.data_ptr()
    p.timesteps = arr([int(t) for t in tab['timesteps']], C.c_int64)
    p.alphas, p.alphas_prev = arr(list(tab['alphas'])), arr(list(tab['alphas_prev']))
    p.sqrt_one_minus_alphas = arr(list(tab['sqrt_one_minus_alphas']))
    p.cfg_scale, p.S, p.B, p.H, p.W, p.flags = 7.5, S, x.shape[0], x.shape[2], x.shape[3], _lib.FLAG_NO_CONTROL
    for k, v in over.items():
        setattr(p, k, arr(*v) if isinstance(v, tuple) else v)
    return p, keep


def test_argument_errors_come_before_any_launch(engine):
    x0, c, uc = _inputs()
    dev = torch.ones(4, *x0.shape, device='cuda')           # any valid device buffer of [S, B,4,H,W]
    out = guarded_out((2, *x0.shape), torch.float32)
    f, i32 = C.c_float, C.c_int32
    bad = {
        'struct_size too small': dict(struct_size=184),
        'struct_size too large': dict(struct_size=200),
        'reserved0 set': dict(reserved0=1),
        'mask without x0': dict(mask=dev.data_ptr(), q_noise=dev.data_ptr(), sqrt_alphas_cumprod_t=([.5] * 4, f),
                                sqrt_one_minus_alphas_cumprod_t=([.5] * 4, f)),
        'mask without q_noise': dict(mask=dev.data_ptr(), x0=dev.data_ptr(), sqrt_alphas_cumprod_t=([.5] * 4, f),
                                     sqrt_one_minus_alphas_cumprod_t=([.5] * 4, f)),
        'mask without coefficients': dict(mask=dev.data_ptr(), x0=dev.data_ptr(), q_noise=dev.data_ptr()),
        'sigma without noise': dict(sigmas=([0.0, 0.1, 0.0, 0.0], f)),
        'log step out of range': dict(n_log=2, log_steps=([0, 4], i32), x_inter_out=out.t.data_ptr()),
        'log step negative': dict(n_log=1, log_steps=([-1], i32), x_inter_out=out.t.data_ptr()),
        'log steps not ascending': dict(n_log=2, log_steps=([1, 1], i32), x_inter_out=out.t.data_ptr()),
        'log steps descending': dict(n_log=2, log_steps=([2, 0], i32), x_inter_out=out.t.data_ptr()),
        'log steps missing': dict(n_log=1, x_inter_out=out.t.data_ptr()),
        'negative n_log': dict(n_log=-1),
        'no steps': dict(S=0),
    }
    for why, over in bad.items():
        x = guarded_out(tuple(x0.shape), torch.float32)
        x.t.copy_(x0)
        p, keep = _params(engine, x.t, c, uc, **over)
        rc = engine.lib.fgdm_sample_ddim_ex(engine.h, C.byref(p), None)
        torch.cuda.synchronize()
        assert rc == ERR_ARG, why
        assert torch.equal(x.t, x0), why
        x.check_guards()
        out.check_guards()
        out.assert_untouched((slice(None),))
        assert b'fgdm_sample_ddim_ex' in engine.lib.fgdm_last_error(engine.h), why
    # the same parameters without the defect run, and zero sigmas need no noise
    x = x0.clone()
    p, keep = _params(engine, x, c, uc, sigmas=([0.0] * 4, f), n_log=2, log_steps=([0, 3], i32), x_inter_out=out.t.data_ptr())
    assert engine.lib.fgdm_sample_ddim_ex(engine.h, C.byref(p), None) == 0
    torch.cuda.synchronize()
    out.check()
    assert torch.equal(out.t[1], x) and not torch.equal(x, x0)          # slot 1: x_prev of the last step
    from fgdm_amd.engine import ContextCachePolicy
    engine._ctx_policy = ContextCachePolicy()                            # the raw calls registered their own context


# ------------------------------------------------------------------------------------------------------------ the kernel alone
@pytest.mark.parametrize('n', [255, 1536, 4096 * 256 + 77])       # odd, the 8 x 16 case, and past one sweep of the 4096-block grid
def test_step_kernel_equals_the_three_kernels_it_fuses(n):
    """one step with a mask, fed fixed e_c / e_u: fgdm_op_ddim_loop_step against mask_blend(axpby(...)) after ddim_step"""
    from fgdm_amd import _lib, engine as E
    lib = _lib.load()
    g = torch.Generator().manual_seed(n)
    r = lambda: torch.randn(n, generator=g)
    x, ec, eu, noise, x0, qn = (guarded_in(r()) for _ in range(6))
    mask = guarded_in((torch.rand(n, generator=g) < 0.5).float() * torch.rand(n, generator=g).round())      # 0 / 1 ...
    mask[::7] = 0.3                                                                                          # ... and soft values
    cfg, a_t, a_prev, sigma, s1m, sa2, s1m2 = 7.5, 0.4047, 0.6411, 0.3127, 0.7716, 0.8007, 0.5991
    xp, p0 = E.ddim_step(x, ec, eu, cfg, a_t, a_prev, sigma, s1m, noise)
    want = E.mask_blend(E.axpby(x0, sa2, qn, s1m2), xp, mask)
    p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
    outs = [guarded_out((n,), torch.float32) for _ in range(5)]
    rc = lib.fgdm_op_ddim_loop_step(p(x), p(ec), p(eu), cfg, a_t, a_prev, sigma, s1m, p(noise), p(mask), p(x0), p(qn), sa2, s1m2,
                                    *[p(o.t) for o in outs], n, None)
    torch.cuda.synchronize()
    assert rc == 0
    x_out, xin_a, xin_b, log_x, log_p0 = (o.check() for o in outs)
    assert torch.equal(log_x, xp) and torch.equal(log_p0, p0)
    assert torch.equal(x_out, want) and torch.equal(xin_a, want) and torch.equal(xin_b, want)
    assert not torch.equal(want, xp)
    # no CFG, no noise, no mask, in place, one input half: ddim_step alone
    xp2, _ = E.ddim_step(x, ec, None, 1.0, a_t, a_prev, 0.0, s1m, None)
    state, half = guarded_out((n,), torch.float32), guarded_out((n,), torch.float32)
    state.t.copy_(x)
    rc = lib.fgdm_op_ddim_loop_step(p(state.t), p(ec), None, 1.0, a_t, a_prev, 0.0, s1m, None, None, None, None, 0.0, 0.0,
                                    p(state.t), p(half.t), None, None, None, n, None)
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(state.check(), xp2) and torch.equal(half.check(), xp2)
    # no update (the launch in front of the first step): the blend of x itself
    want0 = E.mask_blend(E.axpby(x0, sa2, qn, s1m2), x, mask)
    first = guarded_out((n,), torch.float32)
    rc = lib.fgdm_op_ddim_loop_step(p(x), None, None, 0.0, 0.0, 0.0, 0.0, 0.0, None, p(mask), p(x0), p(qn), sa2, s1m2,
                                    None, p(first.t), None, None, None, n, None)
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(first.check(), want0)
