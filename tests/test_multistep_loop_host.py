"""Host side of the device PLMS and DPM-Solver++ loops (fgdm_sample_plms, fgdm_sample_dpmpp), no GPU: the opt-in routing of
PLMSSampler / DPMSolverSampler(model, device_loop=True) with a stand-in engine that records its calls, the tables handed over, the
loops' run order (tests/multistep_loops.py restates the header's description; on the closed-form eps model it must give the
per-step route's trajectory exactly), and the binding against include/fgdm.h."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest
import torch

import kernel_stubs
import multistep_loops as ml
from fgdm_amd import _lib, models, samplers
from test_oracle_golden import analytic_eps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, H, W, TOK = 2, 8, 8, 77
N, P = _lib.FLAG_NO_CONTROL, _lib.FLAG_CFG_PAIRS


class RecEngine(ml.LoopEngine):
    """the loops of multistep_loops.py over the closed-form eps model and the torch stand-ins of the kernels, plus the per-step
    route's apply_model on the same model; every network evaluation is recorded with its timestep"""

    def __init__(self, n_controlnets=0):
        self.calls, self.evals, self.hints = [], [], []
        self.n_controlnets = n_controlnets
        super().__init__(self._net, ml.plms_chain(kernel_stubs), ml.dpmpp_chain(kernel_stubs))

    def _net(self, x, t, ctx):
        self.evals.append(float(t[0]))
        return analytic_eps(x, t, ctx)

    def set_hint(self, cn, hint):
        self.hints.append((cn, hint))

    def apply_model(self, x, t, ctx, control_scales=None, flags=0, pcond=None, out=None):
        self.calls.append((tuple(x.shape), float(t[0]), flags))
        return self._net(x, t, ctx)


class PerStepOnlyEngine(RecEngine):
    """an engine whose library has neither entry"""
    sample_plms = sample_dpmpp = property()


@pytest.fixture()
def stubs(monkeypatch):
    monkeypatch.setattr(samplers, '_k', kernel_stubs)
    monkeypatch.setattr(models, '_k', kernel_stubs)
    monkeypatch.setattr(samplers, '_randn', lambda shape, device: torch.randn(shape))
    monkeypatch.setattr(models, '_randn', lambda shape, device: torch.randn(shape))


def _inputs(seed=3, b=B):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return r(b, 4, H, W), r(b, TOK, 8), r(b, TOK, 8)


def _ldm(engine=None):
    return models.LatentDiffusion(engine=engine or RecEngine(), use_adapter=False)


def _run(sampler, cond, uc=None, scale=1.0, S=4, seed=11, b=B, **kw):
    torch.manual_seed(seed)
    return sampler.sample(S, b, (4, H, W), cond, verbose=False, unconditional_guidance_scale=scale, unconditional_conditioning=uc, **kw)


SAMPLERS = {'plms': samplers.PLMSSampler, 'dpmpp': samplers.DPMSolverSampler}


def _loops(engine, which):
    return engine.plms if which == 'plms' else engine.dpmpp


# ------------------------------------------------------------------------------------------------------------ routing
@pytest.mark.parametrize('which', list(SAMPLERS))
def test_device_loop_is_opt_in_and_takes_a_plain_run(stubs, which):
    x_T, c, uc = _inputs()
    cls = SAMPLERS[which]
    for make in (lambda m: cls(m), lambda m: cls(m, device_loop=False)):
        m = _ldm()
        s = make(m)
        assert s.device_loop is False
        _run(s, c, uc, 7.5, x_T=x_T)
        assert not m.engine.plms and not m.engine.dpmpp
        assert len(m.engine.calls) == (5 if which == 'plms' else 4) and all(k[0] == (2 * B, 4, H, W) and k[2] == N | P for k in m.engine.calls)
    m = _ldm()
    _run(cls(m, device_loop=True), c, uc, 7.5, x_T=x_T)
    assert not m.engine.calls and len(_loops(m.engine, which)) == 1 and not _loops(m.engine, 'dpmpp' if which == 'plms' else 'plms')
    k = _loops(m.engine, which)[0]
    assert k['cond'] is c and k['uncond'] is uc and k['cfg_scale'] == 7.5 and k['flags'] == N | P and k['control_scales'] is None
    # CFG off: no unconditional half, no pair flag
    for uc_, scale in ((None, 7.5), (uc, 1.0)):
        m = _ldm()
        _run(cls(m, device_loop=True), c, uc_, scale, x_T=x_T)
        k = _loops(m.engine, which)[0]
        assert k['uncond'] is None and k['flags'] == N and k['cfg_scale'] == 1.0


class _Corrector:
    def modify_score(self, model, e, x, t, c):
        return e


HOOKS = {
    'callback': dict(callback=lambda i: None),
    'img_callback': dict(img_callback=lambda p, i: None),
    'score_corrector': dict(score_corrector=_Corrector()),
    'noise_dropout': dict(noise_dropout=0.1),
}


@pytest.mark.parametrize('which', list(SAMPLERS))
@pytest.mark.parametrize('hook', list(HOOKS))
def test_each_host_hook_keeps_the_per_step_route(stubs, which, hook):
    x_T, c, uc = _inputs()
    m = _ldm()
    _run(SAMPLERS[which](m, device_loop=True), c, uc, 7.5, x_T=x_T, **HOOKS[hook])
    assert not m.engine.plms and not m.engine.dpmpp and len(m.engine.calls) == (5 if which == 'plms' else 4)


@pytest.mark.parametrize('which', list(SAMPLERS))
def test_conditionings_and_models_the_loop_cannot_hold_keep_the_per_step_route(stubs, which):
    x_T, c, uc = _inputs()
    cls = SAMPLERS[which]

    def per_step(model, cond, ucond=None, scale=1.0):
        _run(cls(model, device_loop=True), cond, ucond, scale, x_T=x_T)
        assert not model.engine.plms and not model.engine.dpmpp and model.engine.calls
    per_step(_ldm(), {'c_crossattn': [c]})                              # a dict cond on a model that is no ControlLDM
    hy = models.LatentDiffusion(engine=RecEngine(), conditioning_key='hybrid')      # hybrid c_concat
    hy.engine.set_concat = lambda cc: None
    per_step(hy, {'c_concat': [torch.rand(B, 5, H, W)], 'c_crossattn': [c]})
    per_step(_ldm(PerStepOnlyEngine()), c, uc, 7.5)                     # an engine without the entry
    sp = _ldm()                                                         # split_input_params: the patch branch of apply_model
    sp.split_input_params = {'ks': (4, 4), 'stride': (4, 4), 'clip_min_weight': 0.01, 'clip_max_weight': 0.5}
    sp.engine.apply_model_patches = lambda x, t, ctx, *a, **k: sp.engine.apply_model(x, t, ctx)
    per_step(sp, c, uc, 7.5)

    class Bare:                                                         # a model that is not backed by an engine
        num_timesteps, parameterization, device = 1000, 'eps', 'cpu'

        def __init__(self):
            ref = _ldm()
            self.betas, self.alphas_cumprod, self.alphas_cumprod_prev = ref.betas, ref.alphas_cumprod, ref.alphas_cumprod_prev
            self.calls = 0

        def apply_model(self, x, t, cc, **kw):
            self.calls += 1
            return 0.1 * x
    bare = Bare()
    _run(cls(bare, device_loop=True), c, uc, 7.5, x_T=x_T)
    assert bare.calls == (5 if which == 'plms' else 4)
    # a ControlLDM with hints (CFG off: the two samplers join no dict conditionings): the hint registered once, the scales handed over
    cm = models.ControlLDM(engine=RecEngine(n_controlnets=1), n_controlnets=1)
    cm.control_scales = [0.5] * 13
    hint = torch.rand(B, 3, 8 * H, 8 * W)
    _run(cls(cm, device_loop=True), {'c_concat': [hint], 'c_crossattn': [c]}, x_T=x_T)
    k = _loops(cm.engine, which)[0]
    assert not cm.engine.calls and cm.engine.hints == [(0, hint)] and k['flags'] == 0 and list(k['control_scales']) == [0.5] * 13
    assert k['cond'] is c and k['uncond'] is None


# ------------------------------------------------------------------------------------------------------------ PLMS tables
def test_plms_tables_timesteps_and_t_next(stubs):
    x_T, c, uc = _inputs()
    m = _ldm()
    s = samplers.PLMSSampler(m, device_loop=True)
    out, inter = _run(s, c, uc, 7.5, S=5, x_T=x_T)
    k = m.engine.plms[0]
    ts = [int(t) for t in s.ddim_timesteps]
    assert k['timesteps'] == ts and len(ts) == 5                                       # ddim_timesteps order
    np.testing.assert_array_equal(k['alphas'], s.ddim_alphas)
    np.testing.assert_array_equal(k['alphas_prev'], s.ddim_alphas_prev)
    np.testing.assert_array_equal(k['sqrt_one_minus_alphas'], s.ddim_sqrt_one_minus_alphas)
    assert 'mask' not in k and k['x_T'] is x_T
    # the walk: t_4, then the second evaluation of the first step at t_next = t_3, then t_3 ... t_0
    assert m.engine.evals == [float(t) for t in (ts[4], ts[3], ts[3], ts[2], ts[1], ts[0])]
    assert inter['x_inter'][0] is x_T and len(inter['x_inter']) == len(inter['pred_x0']) == 3
    # S = 1: the probe's second evaluation runs at the same t (time_range[min(i + 1, len - 1)])
    m = _ldm()
    s = samplers.PLMSSampler(m, device_loop=True)
    _run(s, c, uc, 7.5, S=1, x_T=x_T)
    assert m.engine.plms[0]['timesteps'] == [int(s.ddim_timesteps[0])] and m.engine.evals == [float(s.ddim_timesteps[0])] * 2
    assert m.engine.trace == [(ml.PROBE, 0), (ml.FINISH_FIRST, 0)]


@pytest.mark.parametrize('log_every_t,want', [(1, [0, 1, 2, 3, 4, 5, 6, 7]), (3, [0, 1, 4, 7]), (100, [0, 7])])
def test_plms_log_slots(stubs, log_every_t, want):
    """index % log_every_t == 0 or index == S - 1 with index = S - 1 - i, in walk order; the same lists as the per-step route's"""
    x_T, c, uc = _inputs()
    m, m2 = _ldm(), _ldm()
    out, inter = _run(samplers.PLMSSampler(m, device_loop=True), c, uc, 7.5, S=8, x_T=x_T, log_every_t=log_every_t)
    ref, rinter = _run(samplers.PLMSSampler(m2), c, uc, 7.5, S=8, x_T=x_T, log_every_t=log_every_t)
    assert list(m.engine.plms[0]['log_steps']) == want
    for key in ('x_inter', 'pred_x0'):
        assert len(inter[key]) == len(rinter[key]) == len(want) + 1
        assert all(torch.equal(a, b) for a, b in zip(inter[key], rinter[key]))


def test_plms_tables_original_steps_truncation_and_mask(stubs):
    x_T, c, uc = _inputs()
    m = _ldm()
    s = samplers.PLMSSampler(m, device_loop=True)
    s.make_schedule(5, verbose=False)
    torch.manual_seed(1)
    s.plms_sampling(c, (B, 4, H, W), x_T=x_T, ddim_use_original_steps=True, timesteps=4, log_every_t=1)
    k = m.engine.plms[0]
    assert k['timesteps'] == [0, 1, 2, 3] and list(k['log_steps']) == [0, 1, 2, 3]
    np.testing.assert_array_equal(k['alphas'], m.alphas_cumprod.numpy()[:4])
    np.testing.assert_array_equal(k['alphas_prev'], m.alphas_cumprod_prev.numpy()[:4])
    np.testing.assert_array_equal(k['sqrt_one_minus_alphas'], m.sqrt_one_minus_alphas_cumprod.numpy()[:4])
    # timesteps= on the ddim schedule: the reference's subset (plms.py:125-127), first entries of the tables
    s.make_schedule(20, verbose=False)
    torch.manual_seed(1)
    s.plms_sampling(c, (B, 4, H, W), x_T=x_T, timesteps=10)
    k = m.engine.plms[1]
    assert k['timesteps'] == [int(t) for t in s.ddim_timesteps[:9]] and len(k['alphas']) == 9
    np.testing.assert_array_equal(k['alphas_prev'], s.ddim_alphas_prev[:9])
    # mask: expanded to the latent's shape, q_sample's coefficients per timestep, one q_noise per step
    x0 = torch.randn(B, 4, H, W, generator=torch.Generator().manual_seed(5))
    mask = (torch.arange(W) < W // 2).float().view(1, 1, 1, W)
    _run(s, c, uc, 5.0, x_T=x_T, mask=mask, x0=x0)
    k = m.engine.plms[2]
    assert torch.equal(k['mask'], mask.expand(B, 4, H, W)) and k['x0'] is x0 and tuple(k['q_noise'].shape) == (4, B, 4, H, W)
    h = m._host
    assert k['sqrt_alphas_cumprod_t'] == [h['sqrt_alphas_cumprod'][t] for t in k['timesteps']]
    assert k['sqrt_one_minus_alphas_cumprod_t'] == [h['sqrt_one_minus_alphas_cumprod'][t] for t in k['timesteps']]


# ------------------------------------------------------------------------------------------------------------ DPM tables
def _bits(v):
    return struct.pack('<f', v)


@pytest.mark.parametrize('S', [2, 3, 4, 14, 15, 20])
def test_dpmpp_tables_are_the_coefficients_the_per_step_route_feeds_to_axpby(stubs, monkeypatch, S):
    x_T, c, uc = _inputs()
    m = _ldm()
    _run(samplers.DPMSolverSampler(m, device_loop=True), c, uc, 7.5, S=S, x_T=x_T)
    tab = m.engine.dpmpp[0]['tables']
    assert all(len(tab[k]) == S for k in ('t_float', 'inv_alpha', 'neg_sigma_over_alpha', 'update_kind', 'c1', 'cm0', 'cm1'))
    assert all(isinstance(v, float) and _bits(v) == _bits(struct.unpack('<f', _bits(v))[0]) and float(np.float32(v)) == v
               for k in tab if k != 'update_kind' for v in tab[k])                          # every entry is an fp32 value
    # lower_order_final: below 15 steps the last update is first-order
    second = ml.SECOND
    want = [ml.FIRST] + [second] * (S - 1)
    if S < 15 and S > 1:
        want[-1] = ml.FIRST
    assert tab['update_kind'] == want
    # the per-step route: every axpby call's coefficients, in call order
    seen = []
    import types
    rec = types.SimpleNamespace(**{k: getattr(kernel_stubs, k) for k in dir(kernel_stubs) if not k.startswith('_')})
    rec.axpby = lambda a, ca, b, cb: (seen.append((ca, cb)), kernel_stubs.axpby(a, ca, b, cb))[1]
    monkeypatch.setattr(samplers, '_k', rec)
    m2 = _ldm()
    _run(samplers.DPMSolverSampler(m2), c, uc, 7.5, S=S, x_T=x_T)
    assert [e for e in m2.engine.evals] == tab['t_float'] == m.engine.evals                 # the model's fractional time inputs
    fed = iter(seen)
    for k in range(S):
        ca, cb = next(fed)                                   # data prediction
        assert _bits(ca) == _bits(tab['inv_alpha'][k]) and _bits(cb) == _bits(tab['neg_sigma_over_alpha'][k]), k
        ca, cb = next(fed)                                   # first axpby of the update
        assert _bits(ca) == _bits(tab['c1'][k]) and _bits(cb) == _bits(tab['cm0'][k]), k
        if tab['update_kind'][k] == second:
            ca, cb = next(fed)
            assert ca == 1.0 and _bits(cb) == _bits(tab['cm1'][k]), k
    assert next(fed, None) is None
    # ... and they are what the reference's formulas give in float32 (one spot check: the first-order update to t_1)
    ns = samplers._DiscreteVPSchedule(m.alphas_cumprod.numpy())
    ts = np.linspace(1.0, 1.0 / 1000, S + 1, dtype=np.float32)
    assert _bits(tab['c1'][0]) == _bits(float(ns.marginal_std(ts[1]) / ns.marginal_std(ts[0])))


# ------------------------------------------------------------------------------------------------------------ run order
@pytest.mark.parametrize('S,cfg,masked', [(1, True, False), (2, True, True), (5, True, True), (5, False, False), (8, True, False)])
def test_plms_loop_order_reproduces_the_per_step_trajectory(stubs, S, cfg, masked):
    x_T, c, uc = _inputs()
    kw = dict(log_every_t=1)
    if masked:
        kw.update(mask=(torch.arange(H) % 2 == 0).float().view(1, 1, H, 1), x0=torch.randn(B, 4, H, W, generator=torch.Generator().manual_seed(5)))
    m, m2 = _ldm(), _ldm()
    ref, rinter = _run(samplers.PLMSSampler(m2), c, uc if cfg else None, 7.5, S=S, x_T=x_T, **kw)
    after = torch.randn(3)                                   # where the per-step route leaves the generator
    out, inter = _run(samplers.PLMSSampler(m, device_loop=True), c, uc if cfg else None, 7.5, S=S, x_T=x_T, **kw)
    assert torch.equal(after, torch.randn(3))
    assert len(m.engine.plms) == 1 and not m.engine.calls and not m2.engine.plms
    assert torch.equal(out, ref) and not torch.equal(out, x_T)
    for key in ('x_inter', 'pred_x0'):
        assert len(inter[key]) == len(rinter[key]) == S + 1
        assert all(torch.equal(a, b) for a, b in zip(inter[key], rinter[key])), key
    # probe, finish-first, then Adams-Bashforth of order 1, 2, 3, 3, ...
    assert m.engine.trace == [(ml.PROBE, 0), (ml.FINISH_FIRST, 0)] + [(ml.MULTISTEP, min(i, 3)) for i in range(1, S)]
    assert m.engine.evals == m2.engine.evals and len(m.engine.evals) == S + 1


@pytest.mark.parametrize('S,cfg', [(2, True), (3, True), (4, False), (14, True), (15, True), (20, False)])
def test_dpmpp_loop_order_reproduces_the_per_step_trajectory(stubs, S, cfg):
    x_T, c, uc = _inputs()
    m, m2 = _ldm(), _ldm()
    ref, _ = _run(samplers.DPMSolverSampler(m2), c, uc if cfg else None, 7.5, S=S, x_T=x_T)
    out, none = _run(samplers.DPMSolverSampler(m, device_loop=True), c, uc if cfg else None, 7.5, S=S, x_T=x_T)
    assert none is None and len(m.engine.dpmpp) == 1 and not m.engine.calls
    assert torch.equal(out, ref) and not torch.equal(out, x_T) and m.engine.evals == m2.engine.evals and len(m.engine.evals) == S


# ------------------------------------------------------------------------------------------------------------ binding and header
def _header_struct(hdr, name):
    body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (name, name), hdr, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    return [re.sub(r'\s+', ' ', f).strip() for f in body.split(';') if f.strip()]


@pytest.mark.parametrize('name,cls,size,entry', [('fgdm_plms_params', _lib.FgdmPlmsParams, 168, 'fgdm_sample_plms'),
                                                 ('fgdm_dpmpp_params', _lib.FgdmDpmppParams, 128, 'fgdm_sample_dpmpp')])
def test_binding_and_header_declare_the_entries_and_the_same_structs(name, cls, size, entry):
    res, args = _lib.SIGNATURES[entry]
    assert res is C.c_int and args[1]._type_ is cls
    hdr = open(os.path.join(ROOT, 'include', 'fgdm.h')).read()
    assert re.search(r'\bint\s+%s\s*\(\s*fgdm_engine\*\s*e,\s*const %s\*\s*p,\s*void\*\s*stream\)\s*;' % (entry, name), hdr)
    fields = _header_struct(hdr, name)
    kind = lambda decl: 'ptr' if '*' in decl else decl.rsplit(' ', 1)[0]
    want = {'ptr': C.c_void_p, 'int64_t': C.c_int64, 'int32_t': C.c_int32, 'float': C.c_float}
    assert [f.rsplit(' ', 1)[1].lstrip('*') for f in fields] == [n for n, _ in cls._fields_]
    assert [want[kind(f)] for f in fields] == [t for _, t in cls._fields_]
    assert fields[0] == 'int64_t struct_size' and C.sizeof(cls) == size
    tag = name[len('fgdm_'):-len('_params')].upper()
    assert int(re.search(r'#define FGDM_%s_PARAMS_SIZE_V1 (\d+)' % tag, hdr).group(1)) == size
    assert 'fgdm_op_plms_loop_step' in _lib.SIGNATURES and 'fgdm_op_dpmpp_loop_step' in _lib.SIGNATURES
    assert (_lib.DPMPP_FIRST, _lib.DPMPP_SECOND) == (samplers.DPMPP_FIRST, samplers.DPMPP_SECOND) == (ml.FIRST, ml.SECOND) == tuple(
        int(re.search(r'#define FGDM_DPMPP_%s (\d+)' % w, hdr).group(1)) for w in ('FIRST', 'SECOND'))
    doc = re.sub(r'(\s|\*)+', ' ', hdr)
    for word in ('plms.py:219-223', 'plms.py:224-232', 'dpm_solver.py:386-399', '755-789', 'sampler.py:22-82', 'FGDM_ERR_ARG before any launch'):
        assert word in doc, word


def test_entries_refuse_bad_arguments_without_a_device():
    if not os.path.exists(_lib.LIB_PATH):
        from fgdm_amd import build
        build.build(verbose=False)
    lib = _lib.load()
    for cls, fn in ((_lib.FgdmPlmsParams, lib.fgdm_sample_plms), (_lib.FgdmDpmppParams, lib.fgdm_sample_dpmpp)):
        p = cls()
        p.struct_size = C.sizeof(p)
        assert fn(None, C.byref(p), None) == -1 and fn(None, None, None) == -1
    q, null = C.c_void_p(1 << 20), None
    plms = lambda x=q, ec=q, eu=null, mode=2, order=1, e1=q, e2=null, e3=null, mask=null, x0=null, qn=null, n=64: \
        lib.fgdm_op_plms_loop_step(x, ec, eu, 1.0, mode, order, e1, e2, e3, q, 0.5, 0.6, 0.7, mask, x0, qn, 0.5, 0.5, q, null, null,
                                   null, null, n, null)
    assert plms(x=null) == -1 and plms(n=0) == -1 and plms(ec=null, eu=q) == -1
    assert plms(mask=q) == -1 and plms(mask=q, x0=q) == -1 and plms(mask=q, qn=q) == -1
    assert plms(mode=3) == -1 and plms(mode=-1) == -1 and plms(mode=1, e1=null) == -1
    assert plms(order=0) == -1 and plms(order=4) == -1 and plms(e1=null) == -1 and plms(order=2) == -1 and plms(order=3, e2=q) == -1
    dpm = lambda x=q, ec=q, m1=null, kind=1, n=64: lib.fgdm_op_dpmpp_loop_step(x, ec, null, 1.0, 1.1, -0.2, m1, kind, 0.9, 0.1, 0.05,
                                                                               q, q, null, null, n, null)
    assert dpm(x=null) == -1 and dpm(ec=null) == -1 and dpm(n=0) == -1 and dpm(kind=0) == -1 and dpm(kind=3) == -1 and dpm(kind=2) == -1
