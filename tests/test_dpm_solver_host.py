"""Host side of the DPM-Solver family (fgdm_amd/dpm_solver.py), no GPU: the per-step route against trajectories recorded from the
REFERENCE's own DPM_Solver.sample with the analytic model (tests/golden/dpm_solver.npz, tools/make_dpm_solver_goldens.py), the
invariants of the program both routes read, the refusals, the routing of the device loop, and the drop-in imports.  The one kernel of
the per-step route is replaced by a torch-CPU stand-in (tests/dpm_solver_cases.py) for these tests only; the kernel itself is checked
in tests/test_gpu_dpm_solver_loop.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import dpm_solver_cases as cases
import golden_inputs as gi
import multistep_loops as ml
from common import gold, relerr
from fgdm_amd import _lib, dpm_solver as ds, models, samplers
from oracle import schedule
from test_oracle_golden import analytic_eps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the bound of the existing DPM-Solver++ comparison against the same kind of golden (tests/test_samplers_host.py).  Measured over all
# cases: at most 2.5e-6 (profiles/dpm_solver_parity_errors.txt), so no case needs the wider, measured bound the coefficients'
# expansion could have called for.
TOL = 2e-5


@pytest.fixture()
def stubs(monkeypatch):
    monkeypatch.setattr(ds, '_k', cases.Stubs)
    monkeypatch.setattr(samplers, '_k', cases.Stubs)


@pytest.fixture(scope='module')
def ns():
    return ds.NoiseScheduleVP('discrete', alphas_cumprod=schedule.register_schedule()['alphas_cumprod'])


def _wrapped(ns, model, scale, c, uc):
    return ds.model_wrapper(model, ns, model_type='noise', guidance_type='classifier-free', condition=c, unconditional_condition=uc,
                            guidance_scale=scale)


# ------------------------------------------------------------------------------------------- against the reference
@pytest.mark.parametrize('name', list(cases.CASES))
def test_per_step_route_against_the_reference(stubs, ns, name):
    """final x within TOL of the reference's and exactly its number of network evaluations.  The reference cannot run multistep
    order 3 with lower_order_final below 15 steps (its second-order update unpacks two of three model values: ValueError, recorded
    as '<case>_raises'); there the step before the last is checked against the order-2 solver instead (below)."""
    g = gold('dpm_solver')
    px0, scale, kw = cases.CASES[name]
    x_T, c, uc = gi.get('samp/x_T'), gi.get('samp/c'), gi.get('samp/uc')
    calls = [0]

    def model(x, t, cond):
        calls[0] += 1
        return analytic_eps(x, t, cond)
    out = ds.DPM_Solver(_wrapped(ns, model, scale, c, uc), ns, predict_x0=px0).sample(x_T, **kw)
    if name + '_raises' in g.files:
        assert kw['method'] == 'multistep' and kw['order'] == 3 and kw['steps'] < 15
        assert calls[0] == kw['steps'] and torch.isfinite(out).all()
        return
    err = relerr(out, g[name])
    print(f'{name}: relerr {err:.3e}')
    assert err < TOL, (name, err)
    assert calls[0] == int(g[name + '_calls'][0])


@pytest.mark.parametrize('px0', [True, False])
def test_lower_order_final_of_order_3_ends_like_order_2(ns, px0):
    """multistep order 3, S = 10: the last two updates are the order-2 and the order-1 update over the same times, i.e. the records
    of the order-2 program, history slots aside"""
    p3 = ds.dpm_solver_program(ns, 10, 3, 'time_uniform', 'multistep', px0)
    p2 = ds.dpm_solver_program(ns, 10, 2, 'time_uniform', 'multistep', px0)
    for k in (8, 9):
        assert p3['nterms'][k] == p2['nterms'][k] == (3 if k == 8 else 2)
        assert p3['coef'][k] == p2['coef'][k] and p3['t_float'][k] == p2['t_float'][k]
    assert p3['plane'][8][:3] == [ds.PLANE_M, ds.PLANE_BASE, ds.PLANE_HIST0 + 7 % 3] and p3['nterms'][7] == 4


# ------------------------------------------------------------------------------------------- program invariants
PROGRAMS = [dict(method=m, order=o, steps=S, skip_type=sk, predict_x0=px0, denoise_to_zero=dz, solver_type=st)
            for m in ('multistep', 'singlestep', 'singlestep_fixed') for o in (1, 2, 3) for S in (3, 6, 10, 11, 16)
            for sk in ('time_uniform', 'logSNR') for px0 in (True, False) for dz in (False, True) for st in ('dpm_solver', 'taylor')]


def test_every_program_is_consistent(ns):
    for kw in PROGRAMS:
        p = ds.dpm_solver_program(ns, **kw)
        K = len(p['t_float'])
        nfe = kw['steps'] if kw['method'] != 'singlestep_fixed' else kw['steps'] // kw['order'] * kw['order']
        assert K == nfe + int(kw['denoise_to_zero']), kw
        assert all(len(p[k]) == K for k in p) and all(len(r) == 5 for r in p['plane'] + p['coef'])
        assert ds.program_error(p) is None, (kw, ds.program_error(p))
        written = set()
        for k in range(K):                      # every slot a record reads was written by an earlier record
            n = p['nterms'][k]
            assert 1 <= n <= 5
            for pl in p['plane'][k][:n]:
                assert pl in (ds.PLANE_BASE, ds.PLANE_M) or pl - ds.PLANE_HIST0 in written, (kw, k)
            if p['slot'][k] >= 0:
                written.add(p['slot'][k])
            assert (p['conv_x'][k] == 0.0) == (not kw['predict_x0'] and not (kw['denoise_to_zero'] and k == K - 1))
        assert p['dest'][-1] == ds.DEST_STATE and p['slot'][-1] == -1
        if kw['method'] == 'multistep':
            assert set(p['dest']) == {ds.DEST_STATE}
        assert all(np.isfinite(v) for r in p['coef'] for v in r)


@pytest.mark.parametrize('S', [4, 10, 20])
def test_default_program_has_the_coefficients_of_dpmpp_tables(ns, S):
    """multistep order 2, time_uniform, predict_x0: t_float, the conversion pair and c1, cm0, cm1 of samplers.dpmpp_tables, to fp32
    equality (the program's terms are m0, x, m1 of x' = cm0 m0 + c1 x + cm1 m1)"""
    p = ds.dpm_solver_program(ns, S, 2, 'time_uniform', 'multistep', True)
    tab = samplers.dpmpp_tables(ns, S)
    assert p['t_float'] == tab['t_float'] and p['conv_x'] == tab['inv_alpha'] and p['conv_e'] == tab['neg_sigma_over_alpha']
    for k in range(S):
        second = tab['update_kind'][k] == samplers.DPMPP_SECOND
        assert p['nterms'][k] == (3 if second else 2)
        assert p['plane'][k][:2] == [ds.PLANE_M, ds.PLANE_BASE] and p['coef'][k][:2] == [tab['cm0'][k], tab['c1'][k]]
        if second:
            assert p['plane'][k][2] == ds.PLANE_HIST0 + (k - 1) % 3 and p['coef'][k][2] == tab['cm1'][k]


def test_schedule_inverse_lambda_inverts_lambda(ns):
    for t in (1.0, 0.73, 0.2504, 0.013, 0.001):
        assert abs(float(ns.inverse_lambda(ns.marginal_lambda(t))) - t) < 2e-5 * max(t, 0.05)
    b = ds.NoiseScheduleVP('discrete', betas=torch.linspace(1e-4, 2e-2, 50))
    assert b.total_N == 50 and abs(float(b.marginal_alpha(1.0)) - float(torch.sqrt(torch.cumprod(1 - torch.linspace(1e-4, 2e-2, 50), 0))[-1])) < 1e-6


# ------------------------------------------------------------------------------------------- refusals
def test_refusals_name_what_they_refuse(ns):
    for sched in ('linear', 'cosine'):
        with pytest.raises(NotImplementedError, match=sched):
            ds.NoiseScheduleVP(sched)
    with pytest.raises(ValueError):
        ds.NoiseScheduleVP('sigmoid')
    for mt in ('x_start', 'v', 'score'):
        with pytest.raises(NotImplementedError, match=mt):
            ds.model_wrapper(lambda x, t: x, ns, model_type=mt)
    with pytest.raises(NotImplementedError, match='classifier'):
        ds.model_wrapper(lambda x, t: x, ns, guidance_type='classifier', classifier_fn=lambda *a: None)
    with pytest.raises(NotImplementedError, match='thresholding'):
        ds.DPM_Solver(lambda x, t: x, ns, predict_x0=True, thresholding=True)
    with pytest.raises(NotImplementedError, match='adaptive'):
        ds.DPM_Solver(lambda x, t: x, ns).sample(torch.zeros(1, 4, 8, 8), method='adaptive')
    with pytest.raises(ValueError, match='solver_type'):
        ds.dpm_solver_program(ns, 10, 2, solver_type='heun')
    with pytest.raises(ValueError):
        ds.dpm_solver_program(ns, 10, 4)


def test_program_error_names_the_record(ns):
    p = ds.dpm_solver_program(ns, 4, 2, 'time_uniform', 'multistep', True)
    assert ds.program_error(p) is None
    bad = dict(p, nterms=[2, 6, 3, 3])
    assert 'record 1' in ds.program_error(bad) and 'nterms 6' in ds.program_error(bad)
    bad = dict(p, plane=[[4, 0, 2, 0, 0]] + p['plane'][1:], nterms=[3] + p['nterms'][1:])
    assert 'record 0' in ds.program_error(bad) and 'slot 1' in ds.program_error(bad)
    assert 'destination' in ds.program_error(dict(p, dest=[1, 1, 3, 1]))
    assert 'last record' in ds.program_error(dict(p, dest=[1, 1, 1, 2]))


def test_a_bare_callable_gets_the_continuous_time(stubs, ns):
    seen = []

    def fn(x, t):
        seen.append(float(t[0]))
        return 0.5 * x
    x = torch.randn(1, 4, 8, 8, generator=torch.Generator().manual_seed(0))
    out = ds.DPM_Solver(fn, ns).sample(x, steps=5, order=2, method='multistep')
    assert np.allclose(seen, np.linspace(1.0, 0.001, 6)[:5], rtol=1e-6) and out.shape == x.shape


# ------------------------------------------------------------------------------------------- routing of the device loop
class RecEngine(ml.LoopEngine):
    """records what DPM_Solver hands to sample_dpm_solver and runs the documented loop on the closed-form network; the per-step
    route's apply_model runs the same network"""

    def __init__(self, n_controlnets=0):
        super().__init__(lambda x, t, ctx: analytic_eps(x, t, ctx), None, None)
        self.calls, self.loops, self.hints, self.n_controlnets = [], [], [], n_controlnets

    def set_hint(self, cn, hint):
        self.hints.append((cn, hint))

    def apply_model(self, x, t, ctx, control_scales=None, flags=0, pcond=None, out=None):
        self.calls.append((tuple(x.shape), float(t[0]), flags))
        return self.net(x, t, ctx)

    def sample_dpm_solver(self, x_T, cond, uncond, cfg_scale, program, control_scales=None, flags=0):
        self.loops.append(dict(x_T=x_T, cond=cond, uncond=uncond, cfg_scale=cfg_scale, program=program, control_scales=control_scales,
                               flags=flags))
        return cases.run_device_loop(cases.Stubs.dpm_program_step, self.net, x_T, cond, uncond, cfg_scale, program)


class PerStepOnlyEngine(RecEngine):
    sample_dpm_solver = property()          # a library without the entry


def _inputs(b=2):
    g = torch.Generator().manual_seed(5)
    r = lambda *s: torch.randn(*s, generator=g)
    return r(b, 4, 8, 8), r(b, 77, 8), r(b, 77, 8)


N, P = _lib.FLAG_NO_CONTROL, _lib.FLAG_CFG_PAIRS
KW = dict(steps=6, order=3, method='singlestep')


def test_device_route_is_opt_in_and_hands_over_the_program_of_the_per_step_route(stubs, ns, monkeypatch):
    x_T, c, uc = _inputs()
    m = models.LatentDiffusion(engine=RecEngine(), use_adapter=False)
    ref = ds.DPM_Solver(_wrapped(ns, m, 7.5, c, uc), ns).sample(x_T, **KW)           # off by default
    assert not m.engine.loops and len(m.engine.calls) == 6 and all(k[0] == (4, 4, 8, 8) and k[2] == N | P for k in m.engine.calls)
    seen = []
    real = ds.run_program
    monkeypatch.setattr(ds, 'run_program', lambda prog, fn, x: seen.append(prog) or real(prog, fn, x))
    ds.DPM_Solver(_wrapped(ns, m, 7.5, c, uc), ns).sample(x_T, **KW)
    for model in (m, m.apply_model):                                                 # the mirror, or its bound apply_model
        m.engine.calls.clear(), m.engine.loops.clear()
        out = ds.DPM_Solver(_wrapped(ns, model, 7.5, c, uc), ns, device_loop=True).sample(x_T, **KW)
        assert not m.engine.calls and len(m.engine.loops) == 1
        k = m.engine.loops[0]
        assert k['cond'] is c and k['uncond'] is uc and k['cfg_scale'] == 7.5 and k['flags'] == N | P and k['control_scales'] is None
        assert k['program'] == seen[0] == ds.dpm_solver_program(ns, predict_x0=False, **KW)
        assert torch.equal(out, ref)                                                 # same stand-in kernel, same order: same bits
    for uc_, scale in ((None, 7.5), (uc, 1.0)):                                      # CFG off: no unconditional half, no pair flag
        m.engine.loops.clear()
        ds.DPM_Solver(_wrapped(ns, m, scale, c, uc_), ns, predict_x0=True, device_loop=True).sample(x_T, steps=4, order=2, method='multistep')
        k = m.engine.loops[0]
        assert k['uncond'] is None and k['flags'] == N and k['cfg_scale'] == 1.0


def test_what_the_loop_cannot_hold_keeps_the_per_step_route(stubs, ns):
    x_T, c, uc = _inputs()

    def per_step(fn, model):
        ds.DPM_Solver(fn, ns, device_loop=True).sample(x_T, **KW)
        assert not model.engine.loops and model.engine.calls
    m = models.LatentDiffusion(engine=RecEngine(), use_adapter=False)
    per_step(_wrapped(ns, lambda x, t, cc: m.apply_model(x, t, cc), 7.5, c, uc), m)            # a closure hides the mirror
    m = models.LatentDiffusion(engine=RecEngine(), use_adapter=False)
    per_step(ds.model_wrapper(m, ns, model_kwargs={'cfg_pairs': False}, guidance_type='classifier-free', condition=c,
                              unconditional_condition=uc, guidance_scale=7.5), m)             # model_kwargs
    m = models.LatentDiffusion(engine=PerStepOnlyEngine(), use_adapter=False)
    per_step(_wrapped(ns, m, 7.5, c, uc), m)                                                  # an engine without the entry

    class Own(models.LatentDiffusion):
        def apply_model(self, x, t, cc, **kw):
            return super().apply_model(x, t, cc, **kw)
    m = Own(engine=RecEngine(), use_adapter=False)
    per_step(_wrapped(ns, m, 7.5, c, uc), m)                                                  # a model with its own apply_model
    fn = lambda x, t: analytic_eps(x, (t - 0.001) * 1000., c)
    assert ds.DPM_Solver(fn, ns, device_loop=True)._plan(x_T, ds.dpm_solver_program(ns, **KW)) is None      # a bare callable


def test_control_ldm_takes_the_device_route_unguided(stubs, ns):
    x_T, c, _ = _inputs()
    hint = gi.hint(2, 64, 64)
    m = models.ControlLDM(engine=RecEngine(n_controlnets=1))
    cond = {'c_concat': [hint], 'c_crossattn': [c]}
    ds.DPM_Solver(_wrapped(ns, m, 1.0, cond, None), ns, predict_x0=True, device_loop=True).sample(x_T, steps=3, order=2, method='multistep')
    assert len(m.engine.loops) == 1 and not m.engine.calls and m.engine.hints and m.engine.hints[0][1] is hint
    k = m.engine.loops[0]
    assert k['cond'] is c and k['uncond'] is None and not k['flags'] & (N | P) and k['control_scales'] is not None


# ------------------------------------------------------------------------------------------- drop-in and ABI
def test_dropin_import_paths():
    import fgdm_amd.dropin as dropin
    dropin.install()
    from ldm.models.diffusion.dpm_solver import DPMSolverSampler
    from ldm.models.diffusion.dpm_solver.dpm_solver import NoiseScheduleVP, model_wrapper, DPM_Solver
    from controlnet.ldm.models.diffusion.dpm_solver.dpm_solver import DPM_Solver as Twin
    from controlnet.ldm.models.diffusion.dpm_solver import DPMSolverSampler as TwinSampler
    assert DPMSolverSampler is TwinSampler is samplers.DPMSolverSampler
    assert (NoiseScheduleVP, model_wrapper, DPM_Solver) == (ds.NoiseScheduleVP, ds.model_wrapper, ds.DPM_Solver) and Twin is ds.DPM_Solver


def test_params_struct_and_constants_match_the_header():
    hdr = open(os.path.join(ROOT, 'include', 'fgdm.h')).read()
    assert C.sizeof(_lib.FgdmDpmSolverParams) == int(re.search(r'#define FGDM_DPM_SOLVER_PARAMS_SIZE_V1 (\d+)', hdr).group(1)) == 136
    body = re.search(r'typedef struct fgdm_dpm_solver_params \{(.*?)\} fgdm_dpm_solver_params;', hdr, re.S).group(1)
    names = re.findall(r'(\w+);', body)
    assert names == [f[0] for f in _lib.FgdmDpmSolverParams._fields_]
    want = dict(PLANE_BASE=ds.PLANE_BASE, PLANE_HIST0=ds.PLANE_HIST0, PLANE_M=ds.PLANE_M, DEST_STATE=ds.DEST_STATE, DEST_EVAL=ds.DEST_EVAL)
    for k, v in want.items():
        assert int(re.search(r'#define FGDM_DPM_%s (\d+)' % k, hdr).group(1)) == v == getattr(_lib, 'DPM_' + k)
    assert 'fgdm_sample_dpm_solver' in _lib.SIGNATURES and 'fgdm_op_dpm_program_step' in _lib.SIGNATURES


def test_op_entry_refuses_bad_arguments_before_any_launch():
    """fgdm_op_dpm_program_step returns FGDM_ERR_ARG without touching its pointers (so without a GPU too)"""
    lib = _lib.load()
    q, null = C.c_void_p(1 << 20), None
    pl, cf = (C.c_int32 * 6)(0, 4, 1, 2, 3, 0), (C.c_float * 6)(*[0.5] * 6)

    def call(nterms=2, slot=0, n=64, base=q, h0=q, h1=q, h2=q, planes=pl, coefs=cf, ec=q, xe=q, conv_x=1.0):
        return lib.fgdm_op_dpm_program_step(xe, ec, null, 1.0, conv_x, -0.5, base, h0, h1, h2, slot, nterms, planes, coefs, q, null, null, n, null)
    for bad in (dict(nterms=0), dict(nterms=6), dict(n=0), dict(n=-4), dict(slot=3), dict(slot=-2), dict(base=null), dict(slot=0, h0=null),
                dict(nterms=3, h0=null), dict(nterms=5, h2=null), dict(planes=null), dict(coefs=null), dict(ec=null), dict(xe=null),
                dict(planes=(C.c_int32 * 2)(0, 5)), dict(planes=(C.c_int32 * 2)(-1, 4))):
        assert call(**bad) == -1, bad
