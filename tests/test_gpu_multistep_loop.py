"""The device PLMS and DPM-Solver++ loops (fgdm_sample_plms / k_plms_loop_step, fgdm_sample_dpmpp / k_dpmpp_loop_step) on the GPU.

The yardstick is torch.equal.  The step kernels alone (fgdm_op_plms_loop_step, fgdm_op_dpmpp_loop_step) against the chain of
existing kernels each launch fuses (tests/multistep_loops.py: cfg_combine -> plms_combine / axpby -> ddim_step -> axpby +
mask_blend; cfg_combine -> axpby -> axpby (-> axpby)), on inputs whose dynamic range makes a contracted or a split fma visible
(|e| up to 1e4 against x near 0, scale 9), every output poisoned and guarded (tests/guarded.py).  Then PLMSSampler /
DPMSolverSampler(model, device_loop=True) against the same sampler's per-step route on the same engine from the same generator
state: same networks, same arithmetic rounding for rounding, so there is no tolerance.  Against the reference the loops are run
as the header documents them over the step kernels and the goldens' closed-form eps model (the library's loops evaluate the
engine's own networks, which the goldens do not describe), with the fixtures and tolerances of tests/test_gpu_samplers.py.

The reduced synthetic engine (golden_inputs.SMALL_CFG, one ControlNet) at 8 x 8 latents; the adapter cases need the SD-v1 topology
(the FG-DM adapter exists for no other) and run two steps on one sample.  Neither PLMSSampler nor DPMSolverSampler forwards a
`pcond` on its per-step route (like the reference's, they drop **kwargs), so the adapter reads x on both routes."""
import ctypes as C

import numpy as np
import pytest
import torch

import golden_inputs as gi
import multistep_loops as ml
from common import gold, relerr, report
from fgdm_amd import synth
from guarded import guarded_in, guarded_out

pytestmark = pytest.mark.gpu

ERR_ARG = -1


def _build(cfg, **kw):
    from fgdm_amd.engine import Engine
    e = Engine(cfg, **kw)
    for k, shape in e.param_shapes().items():
        e.load_tensor(k, synth.make_tensor(k, shape))
    e.finalize()
    return e


@pytest.fixture(scope='module')
def engine():
    e = _build(gi.SMALL_CFG, n_controlnets=1)
    yield e
    e.close()


@pytest.fixture(scope='module')
def adapter_engine():
    e = _build(gi.SD_CFG, use_adapter=True)
    yield e
    e.close()


def _guard_engine(e, monkeypatch):
    """every sample_plms / sample_dpmpp of the test runs on guarded buffers, checked when the call returns"""
    real_plms, real_dpm = e.sample_plms, e.sample_dpmpp
    runs = []

    def plms(x_T, *a, **k):
        n_log = len(k.get('log_steps', ()))
        gx = guarded_out(tuple(x_T.shape), torch.float32)
        gi_, gp = (guarded_out((n_log, *x_T.shape), torch.float32) for _ in range(2)) if n_log else (None, None)
        out = real_plms(x_T, *a, **k, out=gx.t, x_inter_out=gi_ and gi_.t, pred_x0_out=gp and gp.t)
        torch.cuda.synchronize()
        for g in (gx, gi_, gp):
            if g is not None:
                g.check()
        runs.append(('plms', n_log))
        return out

    def dpm(x_T, *a, **k):
        gx = guarded_out(tuple(x_T.shape), torch.float32)
        out = real_dpm(x_T, *a, **k, out=gx.t)
        torch.cuda.synchronize()
        gx.check()
        runs.append(('dpmpp', 0))
        return out
    monkeypatch.setattr(e, 'sample_plms', plms)
    monkeypatch.setattr(e, 'sample_dpmpp', dpm)
    return runs


@pytest.fixture()
def guard(engine, monkeypatch):
    return _guard_engine(engine, monkeypatch)


def _ldm(engine):
    from fgdm_amd import models
    return models.LatentDiffusion(gi.SMALL_CFG, engine=engine, use_adapter=False)


def _cldm(engine):
    from fgdm_amd import models
    m = models.ControlLDM(gi.SMALL_CFG, engine=engine, n_controlnets=1)
    m.control_scales = [0.9] * 13
    return m


def _inputs(B=2, H=8, W=8, seed=900):
    x = torch.from_numpy(synth.latents(B, H, W, seed=seed)).cuda()
    c = torch.from_numpy(synth.context(B, seed=seed + 1)).cuda()
    uc = torch.from_numpy(synth.context(B, seed=seed + 2)).cuda()
    return x, c, uc


def _both(make, run, runs, seed=1234):
    """run(sampler) on the per-step route, then on the device loop from the same generator state; the results, bit for bit"""
    outs = []
    for loop in (False, True):
        torch.manual_seed(seed)
        outs.append(run(make(loop)))
    assert len(runs) == 1, 'the device loop did not take this sampling over'
    return outs


def _same(a, b):
    (xa, ia), (xb, ib) = a, b
    assert torch.equal(xa, xb) and bool(torch.isfinite(xa).all())
    if ia is not None or ib is not None:
        for key in ('x_inter', 'pred_x0'):
            assert len(ia[key]) == len(ib[key]), key
            for j, (u, v) in enumerate(zip(ia[key], ib[key])):
                assert torch.equal(u, v), (key, j)
    return xa


def _half_mask(H, W):
    return (torch.arange(W) < W // 2).float().view(1, 1, 1, W).expand(1, 1, H, W).cuda()


# ------------------------------------------------------------------------------------------------------------ whole samplings
# (B, H, W), S, sample()'s keywords, logged steps
PLMS_CASES = {
    'S1_cfg': ((2, 8, 8), 1, dict(scale=7.5), 1),
    'S2_cfg_off': ((2, 8, 8), 2, dict(scale=7.5, uc=False), 2),
    'S5_cfg_log1': ((2, 8, 8), 5, dict(scale=7.5, log_every_t=1), 5),           # reaches order 3
    'S8_cfg_log3': ((2, 8, 8), 8, dict(scale=9.0, log_every_t=3), 4),           # ... and repeats it; index 7, 6, 3, 0
    'S5_mask_cfg': ((2, 8, 8), 5, dict(scale=5.0, mask='half'), 2),
    'S2_mask_scale1_B1': ((1, 8, 8), 2, dict(scale=1.0, mask='half', log_every_t=1), 2),
    'S5_mask_B3_8x16': ((3, 8, 16), 5, dict(scale=7.5, mask='half', log_every_t=3), 3),
}


@pytest.mark.parametrize('name', list(PLMS_CASES))
def test_plms_device_loop_equals_per_step_route(engine, guard, name):
    from fgdm_amd import samplers
    (B, H, W), S, kw, n_logged = PLMS_CASES[name]
    kw = dict(kw)
    x_T, c, uc = _inputs(B, H, W)
    scale, use_uc, mask = kw.pop('scale'), kw.pop('uc', True), kw.pop('mask', None)
    if mask:
        kw['x0'] = torch.from_numpy(synth.latents(B, H, W, seed=911)).cuda()
        kw['mask'] = _half_mask(H, W)
    m = _ldm(engine)
    run = lambda s: s.sample(S, B, (4, H, W), c, verbose=False, x_T=x_T, unconditional_guidance_scale=scale,
                             unconditional_conditioning=uc if use_uc else None, **kw)
    a, b = _both(lambda loop: samplers.PLMSSampler(m, device_loop=loop), run, guard)
    out = _same(a, b)
    assert guard == [('plms', n_logged)] and len(b[1]['x_inter']) == n_logged + 1
    assert not torch.equal(out, x_T)


def test_plms_original_steps_through_plms_sampling(engine, guard):
    from fgdm_amd import samplers
    x_T, c, uc = _inputs()
    m = _ldm(engine)

    def run(s):
        s.make_schedule(5, verbose=False)
        return s.plms_sampling(c, (2, 4, 8, 8), x_T=x_T, ddim_use_original_steps=True, timesteps=6, log_every_t=2,
                               unconditional_guidance_scale=7.5, unconditional_conditioning=uc)
    a, b = _both(lambda loop: samplers.PLMSSampler(m, device_loop=loop), run, guard)
    _same(a, b)
    assert guard == [('plms', 4)]          # index 5, 4, 2 and 0 of the six steps


DPM_CASES = {
    'S2_cfg': ((2, 8, 8), 2, dict(scale=7.5)),
    'S3_cfg_off_B1': ((1, 8, 8), 3, dict(scale=7.5, uc=False)),
    'S4_cfg_B3': ((3, 8, 8), 4, dict(scale=9.0)),             # lower_order_final: the last update is first-order
    'S15_cfg_B1': ((1, 8, 8), 15, dict(scale=7.5)),           # ... and from 15 steps on it is not
    'S16_scale1': ((2, 8, 8), 16, dict(scale=1.0)),
}


@pytest.mark.parametrize('name', list(DPM_CASES))
def test_dpmpp_device_loop_equals_per_step_route(engine, guard, name):
    from fgdm_amd import samplers
    (B, H, W), S, kw = DPM_CASES[name]
    x_T, c, uc = _inputs(B, H, W)
    m = _ldm(engine)
    run = lambda s: s.sample(S, B, (4, H, W), c, verbose=False, x_T=x_T, unconditional_guidance_scale=kw['scale'],
                             unconditional_conditioning=uc if kw.get('uc', True) else None)
    a, b = _both(lambda loop: samplers.DPMSolverSampler(m, device_loop=loop), run, guard)
    out = _same(a, b)
    assert guard == [('dpmpp', 0)] and not torch.equal(out, x_T)


@pytest.mark.parametrize('which', ['plms', 'dpmpp'])
def test_control_ldm_with_hints(engine, guard, which):
    """(CFG off: neither sampler joins two dict conditionings into one batch, on either route)"""
    from fgdm_amd import samplers
    x_T, c, _ = _inputs()
    hint = torch.from_numpy(synth.hint(2, res=64, seed=903)).cuda()
    m = _cldm(engine)
    cls = samplers.PLMSSampler if which == 'plms' else samplers.DPMSolverSampler
    run = lambda s, h=hint: s.sample(4, 2, (4, 8, 8), {'c_concat': [h], 'c_crossattn': [c]}, verbose=False, x_T=x_T)
    a, b = _both(lambda loop: cls(m, device_loop=loop), run, guard)
    out = _same(a, b)
    torch.manual_seed(1234)                                      # ... and the hint matters
    moved = run(cls(m, device_loop=True), hint.flip(-1).contiguous())[0]
    assert not torch.equal(moved, out)


@pytest.mark.parametrize('which', ['plms', 'dpmpp'])
def test_adapter_model(adapter_engine, monkeypatch, which):
    from fgdm_amd import models, samplers
    runs = _guard_engine(adapter_engine, monkeypatch)
    x_T, c, uc = _inputs(B=1)
    m = models.LatentDiffusion(gi.SD_CFG, engine=adapter_engine, use_adapter=True)
    cls = samplers.PLMSSampler if which == 'plms' else samplers.DPMSolverSampler
    run = lambda s: s.sample(2, 1, (4, 8, 8), c, verbose=False, x_T=x_T, unconditional_guidance_scale=7.5, unconditional_conditioning=uc)
    a, b = _both(lambda loop: cls(m, device_loop=loop), run, runs)
    _same(a, b)


# ------------------------------------------------------------------------------------------------------------ the kernels alone
def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def plms_op(lib, null=()):
    """multistep_loops' step() as ONE launch of fgdm_op_plms_loop_step on poisoned, guarded outputs.  null: outputs handed over as
    NULL.  Outputs the mode must not write (the probe's x_out and logs) are checked to be untouched."""
    def step(x, ec, eu, cfg, mode, order, hist, a_t, a_prev, s1m, blend):
        shape = tuple(x.shape)
        outs = {k: None if k in null else guarded_out(shape, torch.float32) for k in ('e_out', 'x_out', 'xin_a', 'xin_b', 'log_x', 'log_p0')}
        mask, x0, qn, sa, s1m_n = blend if blend is not None else (None, None, None, 0.0, 0.0)
        ptr = lambda k: _p(outs[k] and outs[k].t)
        rc = lib.fgdm_op_plms_loop_step(_p(x), _p(ec), _p(eu), cfg, mode, order, *[_p(h) for h in hist], ptr('e_out'), a_t, a_prev, s1m,
                                        _p(mask), _p(x0), _p(qn), sa, s1m_n, ptr('x_out'), ptr('xin_a'), ptr('xin_b'), ptr('log_x'),
                                        ptr('log_p0'), x.numel(), None)
        torch.cuda.synchronize()
        assert rc == 0
        written = {'e_out': ec is not None, 'x_out': ec is None or mode != ml.PROBE, 'xin_a': True, 'xin_b': True,
                   'log_x': ec is not None and mode != ml.PROBE, 'log_p0': ec is not None and mode != ml.PROBE}
        got = {}
        for k, g in outs.items():
            if g is None:
                got[k] = None
            elif written[k]:
                got[k] = g.check()
            else:
                g.check_guards()
                g.assert_untouched((slice(None),))
                got[k] = None
        if got['xin_a'] is not None and got['xin_b'] is not None:
            assert torch.equal(got['xin_a'], got['xin_b'])
        return got['e_out'], got['x_out'], got['xin_a'] if got['xin_a'] is not None else got['xin_b'], got['log_x'], got['log_p0']
    return step


def dpmpp_op(lib, null=()):
    def step(x, ec, eu, cfg, inv_alpha, nsa, m1, kind, c1, cm0, cm1):
        outs = {k: None if k in null else guarded_out(tuple(x.shape), torch.float32) for k in ('m0_out', 'x_out', 'xin_a', 'xin_b')}
        ptr = lambda k: _p(outs[k] and outs[k].t)
        rc = lib.fgdm_op_dpmpp_loop_step(_p(x), _p(ec), _p(eu), cfg, inv_alpha, nsa, _p(m1), kind, c1, cm0, cm1, ptr('m0_out'),
                                         ptr('x_out'), ptr('xin_a'), ptr('xin_b'), x.numel(), None)
        torch.cuda.synchronize()
        assert rc == 0
        got = {k: None if g is None else g.check() for k, g in outs.items()}
        for k in ('xin_a', 'xin_b'):
            if got[k] is not None and got['x_out'] is not None:
                assert torch.equal(got[k], got['x_out'])
        return got['m0_out'], got['x_out'] if got['x_out'] is not None else got['xin_a']
    return step


def _wide(n, g, scale_lo=-2.0, scale_hi=4.0):
    """randn times 10 ** U(lo, hi): magnitudes from 1e-2 up to 1e4 side by side"""
    return torch.randn(n, generator=g) * 10.0 ** (scale_lo + (scale_hi - scale_lo) * torch.rand(n, generator=g))


# 4 * (256 * 3 + 1): three full blocks and a tail; 255 / 1536 / 4096 * 256 + 77: the sizes of the DDIM loop's step-kernel test
SIZES = [4, 60, 1020, 1024, 4 * (256 * 3 + 1), 255, 1536, 4096 * 256 + 77]


def _eq(got, want, what):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert (g is None) == (w is None) and (g is None or torch.equal(g, w)), (what, k)


@pytest.mark.parametrize('n', SIZES)
def test_plms_step_kernel_equals_the_kernels_it_fuses(n):
    from fgdm_amd import _lib, engine as E
    lib = _lib.load()
    g = torch.Generator().manual_seed(n)
    x = guarded_in(torch.randn(n, generator=g) * 1e-3)                                  # x near 0 against |e| up to 1e4
    ec, eu, e1, e2, e3 = (guarded_in(_wide(n, g)) for _ in range(5))
    x0, qn = (guarded_in(torch.randn(n, generator=g)) for _ in range(2))
    mask = (torch.rand(n, generator=g) < 0.5).float()
    mask[::7] = 0.3                                                                      # 0 / 1 and soft values
    mask = guarded_in(mask)
    cfg, a_t, a_prev, s1m, sa2, s1m2 = 9.0, 0.4047, 0.6411, 0.7716, 0.8007, 0.5991
    chain, op = ml.plms_chain(E), plms_op(lib)
    blend = (mask, x0, qn, sa2, s1m2)
    hist = (e1, e2, e3)
    for mode, order in ((ml.PROBE, 0), (ml.FINISH_FIRST, 0), (ml.MULTISTEP, 1), (ml.MULTISTEP, 2), (ml.MULTISTEP, 3)):
        h = tuple(v if j < max(order, 1) and mode != ml.PROBE else None for j, v in enumerate(hist))
        for u in (eu, None):
            for bl in (blend, None):
                args = (x, ec, u, cfg, mode, order, h, a_t, a_prev, s1m, bl if mode != ml.PROBE else None)
                want = chain(*args)
                _eq(op(*args), want, (mode, order, u is not None, bl is not None))
                if mode != ml.PROBE:       # without the log pointers, and with one input half only: the other outputs are the same
                    got = plms_op(lib, null=('log_x', 'log_p0', 'xin_b'))(*args)
                    _eq(got, want[:3] + (None, None), (mode, order, 'no logs'))
    # the five modes / orders differ in what they compute
    assert len({tuple(chain(x, ec, eu, cfg, m, o, hist, a_t, a_prev, s1m, None)[2][:4].tolist())
                for m, o in ((0, 0), (1, 0), (2, 1), (2, 2), (2, 3))}) == 5
    # no update (the launch in front of the first step): the blend of x itself, nothing else written
    want0 = E.mask_blend(E.axpby(x0, sa2, qn, s1m2), x, mask)
    got = plms_op(lib, null=('e_out', 'log_x', 'log_p0'))(x, None, None, 0.0, 0, 0, (None,) * 3, 0.0, 0.0, 0.0, blend)
    assert torch.equal(got[1], want0) and torch.equal(got[2], want0)
    # in place, as the loop runs it: x_out is the state, e_out the plane of e3 (order 3 replaces the oldest plane)
    want = chain(x, ec, eu, cfg, ml.MULTISTEP, 3, hist, a_t, a_prev, s1m, blend)
    state, plane, half = (guarded_out((n,), torch.float32) for _ in range(3))
    state.t.copy_(x)
    plane.t.copy_(e3)
    rc = lib.fgdm_op_plms_loop_step(_p(state.t), _p(ec), _p(eu), cfg, ml.MULTISTEP, 3, _p(e1), _p(e2), _p(plane.t), _p(plane.t), a_t, a_prev,
                                    s1m, _p(mask), _p(x0), _p(qn), sa2, s1m2, _p(state.t), _p(half.t), None, None, None, n, None)
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(plane.check(), want[0]) and torch.equal(state.check(), want[1]) and torch.equal(half.check(), want[1])


@pytest.mark.parametrize('n', SIZES)
def test_dpmpp_step_kernel_equals_the_kernels_it_fuses(n):
    from fgdm_amd import _lib, engine as E
    lib = _lib.load()
    g = torch.Generator().manual_seed(n + 1)
    x = guarded_in(torch.randn(n, generator=g) * 1e-3)
    ec, eu, m1 = (guarded_in(_wide(n, g)) for _ in range(3))
    # coefficients of the size the 20-step tables hold, none of them a power of two
    cfg, ia, nsa, c1, cm0, cm1 = 9.0, 1.3971, -0.9757, 0.8312, 0.2714, -0.0931
    chain, op = ml.dpmpp_chain(E), dpmpp_op(lib)
    for kind, prev in ((ml.FIRST, None), (ml.FIRST, m1), (ml.SECOND, m1)):        # (FIRST, None): the first evaluation
        for u in (eu, None):
            args = (x, ec, u, cfg, ia, nsa, prev, kind, c1, cm0, cm1)
            want = chain(*args)
            _eq(op(*args), want, (kind, prev is not None, u is not None))
            got = dpmpp_op(lib, null=('m0_out', 'xin_b'))(*args)
            assert got[0] is None and torch.equal(got[1], want[1])
    assert not torch.equal(chain(x, ec, eu, cfg, ia, nsa, m1, ml.FIRST, c1, cm0, cm1)[1], chain(x, ec, eu, cfg, ia, nsa, m1, ml.SECOND, c1, cm0, cm1)[1])
    # in place, as the loop runs it: x_out is the state
    want = chain(x, ec, eu, cfg, ia, nsa, m1, ml.SECOND, c1, cm0, cm1)
    state, plane = guarded_out((n,), torch.float32), guarded_out((n,), torch.float32)
    state.t.copy_(x)
    rc = lib.fgdm_op_dpmpp_loop_step(_p(state.t), _p(ec), _p(eu), cfg, ia, nsa, _p(m1), ml.SECOND, c1, cm0, cm1, _p(plane.t), _p(state.t),
                                     None, None, n, None)
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(plane.check(), want[0]) and torch.equal(state.check(), want[1])


# ------------------------------------------------------------------------------------------------------------ against the reference
@pytest.fixture()
def cpu_noise(monkeypatch):
    """draw sampler noise from the CPU generator (as the reference run that produced the goldens did)"""
    from fgdm_amd import models, samplers
    monkeypatch.setattr(samplers, '_randn', lambda shape, device: torch.randn(shape).to(device))
    monkeypatch.setattr(models, '_randn', lambda shape, device: torch.randn(shape).to(device))
    monkeypatch.setattr(torch, 'randn_like', lambda x, **k: torch.randn(x.shape).to(x.device))


def _golden_model():
    """a LatentDiffusion mirror whose engine runs the documented loops over the step kernels and the goldens' closed-form eps"""
    from fgdm_amd import _lib, models
    from test_oracle_golden import analytic_eps
    lib = _lib.load()
    return models.LatentDiffusion(engine=ml.LoopEngine(analytic_eps, plms_op(lib), dpmpp_op(lib), device='cuda'), use_adapter=False)


def test_loops_reproduce_the_reference_golden_trajectories(cpu_noise):
    from fgdm_amd import samplers
    from test_gpu_samplers import STOL
    g, g2 = gold('samplers'), gold('samplers2')
    x_T, c, uc = (gi.get(k).cuda() for k in ('samp/x_T', 'samp/c', 'samp/uc'))
    m = _golden_model()
    out, _ = samplers.PLMSSampler(m, device_loop=True).sample(50, 2, (4, 8, 8), conditioning=c, x_T=x_T, eta=0.0, verbose=False,
                                                              unconditional_guidance_scale=7.5, unconditional_conditioning=uc)
    assert len(m.engine.plms) == 1 and len(m.engine.trace) == 51
    assert report('PLMS device loop S50 (step kernel) vs reference', relerr(out.cpu(), g['plms_S50']), STOL) < STOL
    for S, scale in ((20, 7.5), (10, 7.5), (12, 1.0)):              # the cases and the 5e-5 of test_dpm_solver_and_encode_on_device
        m = _golden_model()
        out, _ = samplers.DPMSolverSampler(m, device_loop=True).sample(S, 2, (4, 8, 8), conditioning=c, x_T=x_T, verbose=False,
                                                                       unconditional_guidance_scale=scale, unconditional_conditioning=uc)
        assert len(m.engine.dpmpp) == 1
        assert report(f'DPM-Solver++ device loop S{S} scale {scale} (step kernel) vs reference',
                      relerr(out.cpu(), g2[f'dpm_S{S}_s{scale}']), 5e-5) < 5e-5


# ------------------------------------------------------------------------------------------------------------ argument errors
def _arr(keep, v, ty=C.c_float):
    keep.append((ty * len(v))(*[ty(x).value for x in v]))
    return C.cast(keep[-1], C.c_void_p)


def _plms_params(x_, c_, uc_, **over):
    from fgdm_amd import _lib
    from oracle import schedule
    S = 4
    tab = schedule.ddim_tables(schedule.register_schedule()['alphas_cumprod'], S, 0.0)
    keep = []
    p = _lib.FgdmPlmsParams()
    p.struct_size = C.sizeof(p)
    p.x, p.cond, p.uncond = x_.data_ptr(), c_.data_ptr(), uc_.data_ptr()
    p.timesteps = _arr(keep, [int(t) for t in tab['timesteps']], C.c_int64)
    p.alphas, p.alphas_prev = _arr(keep, list(tab['alphas'])), _arr(keep, list(tab['alphas_prev']))
    p.sqrt_one_minus_alphas = _arr(keep, list(tab['sqrt_one_minus_alphas']))
    p.cfg_scale, p.S, p.B, p.H, p.W, p.flags = 7.5, S, x_.shape[0], x_.shape[2], x_.shape[3], _lib.FLAG_NO_CONTROL
    for k, v in over.items():
        setattr(p, k, _arr(keep, *v) if isinstance(v, tuple) else v)
    return p, keep


def _dpmpp_params(x_, c_, uc_, **over):
    from fgdm_amd import _lib, samplers
    from oracle import schedule
    tab = samplers.dpmpp_tables(samplers._DiscreteVPSchedule(schedule.register_schedule()['alphas_cumprod']), 4)
    keep = []
    p = _lib.FgdmDpmppParams()
    p.struct_size = C.sizeof(p)
    p.x, p.cond, p.uncond = x_.data_ptr(), c_.data_ptr(), uc_.data_ptr()
    for name in ('t_float', 'inv_alpha', 'neg_sigma_over_alpha', 'c1', 'cm0', 'cm1'):
        setattr(p, name, _arr(keep, tab[name]))
    p.update_kind = _arr(keep, tab['update_kind'], C.c_int32)
    p.cfg_scale, p.n_eval, p.B, p.H, p.W, p.flags = 7.5, 4, x_.shape[0], x_.shape[2], x_.shape[3], _lib.FLAG_NO_CONTROL
    for k, v in over.items():
        setattr(p, k, _arr(keep, *v) if isinstance(v, tuple) else v)
    return p, keep


def _refused(engine, entry, make, bad, x0, c, uc, out=None):
    for why, over in bad.items():
        x = guarded_out(tuple(x0.shape), torch.float32)
        x.t.copy_(x0)
        p, keep = make(x.t, c, uc, **over)
        rc = getattr(engine.lib, entry)(engine.h, C.byref(p), None)
        torch.cuda.synchronize()
        assert rc == ERR_ARG, why
        assert torch.equal(x.t, x0), why
        x.check_guards()
        if out is not None:
            out.check_guards()
            out.assert_untouched((slice(None),))
        assert entry.encode() in engine.lib.fgdm_last_error(engine.h), why


def test_plms_argument_errors_come_before_any_launch(engine):
    from fgdm_amd.engine import ContextCachePolicy
    x0, c, uc = _inputs()
    dev = torch.ones(4, *x0.shape, device='cuda')           # any valid device buffer of [S, B,4,H,W]
    out = guarded_out((2, *x0.shape), torch.float32)
    f, i32 = C.c_float, C.c_int32
    coef = dict(sqrt_alphas_cumprod_t=([.5] * 4, f), sqrt_one_minus_alphas_cumprod_t=([.5] * 4, f))
    bad = {
        'struct_size too small': dict(struct_size=160),
        'struct_size too large': dict(struct_size=176),
        'reserved0 set': dict(reserved0=1),
        'x NULL': dict(x=None),
        'cond NULL': dict(cond=None),
        'timesteps NULL': dict(timesteps=None),
        'alphas NULL': dict(alphas=None),
        'alphas_prev NULL': dict(alphas_prev=None),
        'sqrt_one_minus_alphas NULL': dict(sqrt_one_minus_alphas=None),
        'no steps': dict(S=0),
        'B = 0': dict(B=0),
        'H < 0': dict(H=-8),
        'W = 0': dict(W=0),
        'mask without x0': dict(mask=dev.data_ptr(), q_noise=dev.data_ptr(), **coef),
        'mask without q_noise': dict(mask=dev.data_ptr(), x0=dev.data_ptr(), **coef),
        'mask without coefficients': dict(mask=dev.data_ptr(), x0=dev.data_ptr(), q_noise=dev.data_ptr()),
        'log step out of range': dict(n_log=2, log_steps=([0, 4], i32), x_inter_out=out.t.data_ptr()),
        'log step negative': dict(n_log=1, log_steps=([-1], i32), x_inter_out=out.t.data_ptr()),
        'log steps not ascending': dict(n_log=2, log_steps=([1, 1], i32), x_inter_out=out.t.data_ptr()),
        'log steps missing': dict(n_log=1, x_inter_out=out.t.data_ptr()),
        'negative n_log': dict(n_log=-1),
    }
    _refused(engine, 'fgdm_sample_plms', _plms_params, bad, x0, c, uc, out)
    # the same parameters without the defect run
    x = x0.clone()
    p, keep = _plms_params(x, c, uc, n_log=2, log_steps=([0, 3], i32), x_inter_out=out.t.data_ptr())
    assert engine.lib.fgdm_sample_plms(engine.h, C.byref(p), None) == 0
    torch.cuda.synchronize()
    out.check()
    assert torch.equal(out.t[1], x) and not torch.equal(x, x0)          # slot 1: x_prev of the last step
    engine._ctx_policy = ContextCachePolicy()                            # the raw calls registered their own context


def test_dpmpp_argument_errors_come_before_any_launch(engine):
    from fgdm_amd.engine import ContextCachePolicy
    x0, c, uc = _inputs()
    i32 = C.c_int32
    bad = {
        'struct_size too small': dict(struct_size=120),
        'struct_size too large': dict(struct_size=136),
        'reserved0 set': dict(reserved0=1),
        'reserved1 set': dict(reserved1=1),
        'x NULL': dict(x=None),
        'cond NULL': dict(cond=None),
        'no evaluations': dict(n_eval=0),
        'B = 0': dict(B=0),
        'H = 0': dict(H=0),
        'W < 0': dict(W=-8),
        'update_kind 0': dict(update_kind=([1, 2, 0, 1], i32)),
        'update_kind 3': dict(update_kind=([1, 3, 2, 1], i32)),
        'second order at evaluation 0': dict(update_kind=([2, 2, 2, 1], i32)),
    }
    bad.update({f'{k} NULL': {k: None} for k in ('t_float', 'inv_alpha', 'neg_sigma_over_alpha', 'update_kind', 'c1', 'cm0', 'cm1')})
    _refused(engine, 'fgdm_sample_dpmpp', _dpmpp_params, bad, x0, c, uc)
    x = x0.clone()
    p, keep = _dpmpp_params(x, c, uc)
    assert engine.lib.fgdm_sample_dpmpp(engine.h, C.byref(p), None) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(x).all()) and not torch.equal(x, x0)
    engine._ctx_policy = ContextCachePolicy()
