"""Host side of the device ancestral loop and the device DDIM inversion (fgdm_sample_ancestral, fgdm_ddim_encode), no GPU: the
segment planner, the opt-in routing of LatentDiffusion / ControlLDM(device_loop=True).p_sample_loop and of
ControlDDIMSampler(device_loop=True).encode with a stand-in engine that records its calls, the order in which the pre-drawn noise
is consumed, the loops' run order (tests/ancestral_loops.py restates the header's description; on the closed-form eps model it
must give the per-step route's trajectory exactly), the shared encode tables, and the binding against include/fgdm.h."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest
import torch

import ancestral_loops as al
import kernel_stubs
from fgdm_amd import _lib, models, samplers
from test_oracle_golden import analytic_eps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, H, W, TOK = 2, 8, 8, 77
N = _lib.FLAG_NO_CONTROL


class RecEngine(al.WalkEngine):
    """the loops of ancestral_loops.py over the closed-form eps model and the torch stand-ins of the kernels, plus the per-step
    route's apply_model on the same model; every network evaluation is recorded with its timestep"""

    def __init__(self, n_controlnets=0):
        self.calls, self.evals, self.hints = [], [], []
        self.n_controlnets = n_controlnets
        super().__init__(self._net, al.ancestral_chain(kernel_stubs), al.invert_chain(kernel_stubs))

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
    sample_ancestral = ddim_encode = property()


@pytest.fixture()
def draws(monkeypatch):
    """the kernels' torch stand-ins, and every noise draw recorded as (who, shape) in the order it happens"""
    seen = []

    def randn(shape, device):
        seen.append(('randn', tuple(shape)))
        return torch.randn(shape)

    def randn_like(x, **k):
        seen.append(('randn_like', tuple(x.shape)))
        return torch.randn(x.shape)
    monkeypatch.setattr(samplers, '_k', kernel_stubs)
    monkeypatch.setattr(models, '_k', kernel_stubs)
    monkeypatch.setattr(samplers, '_randn', randn)
    monkeypatch.setattr(models, '_randn', randn)
    monkeypatch.setattr(torch, 'randn_like', randn_like)
    return seen


def _inputs(seed=3, b=B):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return r(b, 4, H, W), r(b, TOK, 8), r(b, TOK, 8)


def _ldm(engine=None, **kw):
    return models.LatentDiffusion(engine=engine or RecEngine(), use_adapter=False, **kw)


def _loop(m, cond, seed=11, b=B, **kw):
    torch.manual_seed(seed)
    return m.p_sample_loop(cond, (b, 4, H, W), **kw)


# ------------------------------------------------------------------------------------------------------------ the segment planner
@pytest.mark.parametrize('S,step,bound', [(1, 4096, 256 << 20), (6, 4096, 3 * 4096), (6, 4096, 2 * 4096 + 1), (7, 4096, 3 * 4096),
                                          (1000, 16 * 4 * 64 * 64 * 4, 256 << 20), (5, 4096, 4095), (5, 4096, 0), (6, 4096, 6 * 4096)])
def test_segments_cover_the_walk_once_in_order_within_the_bound(S, step, bound):
    segs = models.plan_noise_segments(S, step, bound)
    assert [i for a, b in segs for i in range(a, b)] == list(range(S))          # exactly once, in order
    assert all(b > a for a, b in segs)
    if step <= bound:
        assert all((b - a) * step <= bound for a, b in segs)
        assert len(segs) == -(-S // (bound // step))                            # no more segments than the bound asks for
    else:
        assert segs == [(i, i + 1) for i in range(S)]                           # one step already exceeds the bound
    if S * step <= bound:
        assert segs == [(0, S)]


def test_the_default_bound_is_256_mib_and_splits_the_long_walk():
    m = _ldm()
    assert m.max_loop_noise_bytes == 256 << 20 and m.device_loop is False
    step = 16 * 4 * 64 * 64 * 4
    segs = models.plan_noise_segments(1000, step, m.max_loop_noise_bytes)
    assert segs[0] == (0, 256) and segs[-1] == (768, 1000) and len(segs) == 4
    assert models.plan_noise_segments(1000, 2 * step, m.max_loop_noise_bytes)[0] == (0, 128)      # a mask doubles a step's noise


# ------------------------------------------------------------------------------------------------------------ routing
def test_device_loop_is_opt_in_and_takes_a_plain_run(draws):
    x_T, c, _ = _inputs()
    for m in (_ldm(), _ldm(device_loop=False)):
        _loop(m, c, x_T=x_T, timesteps=5)
        assert not m.engine.ancestral and len(m.engine.calls) == 5 and all(k[0] == (B, 4, H, W) and k[2] == N for k in m.engine.calls)
    m = _ldm(device_loop=True)
    out = _loop(m, c, x_T=x_T, timesteps=5)
    assert not m.engine.calls and len(m.engine.ancestral) == 1
    k = m.engine.ancestral[0]
    assert k['cond'] is c and k['flags'] == N and k['control_scales'] is None and k['timesteps'] == [4, 3, 2, 1, 0]
    assert k['mask'] is None and k['x0'] is None and k['q_noise'] is None and tuple(k['step_noise'].shape) == (5, B, 4, H, W)
    assert m.engine.evals == [4.0, 3.0, 2.0, 1.0, 0.0] and torch.is_tensor(out)
    # the tables: walk order, the per-step route's expressions
    h = m._host
    for name in ('sqrt_recip_alphas_cumprod', 'sqrt_recipm1_alphas_cumprod', 'posterior_mean_coef1', 'posterior_mean_coef2'):
        assert k['tables'][name] == [float(h[name][t]) for t in (4, 3, 2, 1, 0)]
    assert k['tables']['std'] == [float(np.exp(0.5 * h['posterior_log_variance_clipped'][t])) for t in (4, 3, 2, 1)] + [0.0]
    # sample() goes through the same loop; a {'c_crossattn': [ctx]} cond is the tensor
    m = _ldm(device_loop=True)
    torch.manual_seed(1)
    m.sample({'c_crossattn': [c]}, batch_size=B, x_T=x_T, timesteps=3, shape=(B, 4, H, W))
    assert len(m.engine.ancestral) == 1 and torch.equal(m.engine.ancestral[0]['cond'], c) and not m.engine.calls


HOST_NEEDS = {
    'callback': dict(callback=lambda i: None),
    'img_callback': dict(img_callback=lambda x, i: None),
    'noise': dict(noise=torch.zeros(B, 4, H, W)),
    'use_original': dict(use_original=True),
}


@pytest.mark.parametrize('what', list(HOST_NEEDS))
def test_each_host_need_keeps_the_per_step_route(draws, what):
    x_T, c, _ = _inputs()
    m = _ldm(device_loop=True)
    _loop(m, c, x_T=x_T, timesteps=4, **HOST_NEEDS[what])
    assert not m.engine.ancestral and len(m.engine.calls) == 4


def test_return_x0_keeps_the_per_step_route(draws):
    """p_sample(return_x0=True) returns a pair, which is p_sample's business; what matters is that the device loop declines"""
    x_T, c, _ = _inputs()
    m = _ldm(device_loop=True)
    with pytest.raises(AttributeError):                       # the second step is handed the pair
        _loop(m, c, x_T=x_T, timesteps=2, return_x0=True)
    assert not m.engine.ancestral and m.engine.calls


def test_conditionings_and_models_the_loop_cannot_hold_keep_the_per_step_route(draws):
    x_T, c, _ = _inputs()

    def per_step(model, cond, **kw):
        _loop(model, cond, x_T=x_T, timesteps=3, **kw)
        assert not model.engine.ancestral and len(model.engine.calls) == 3
    hy = models.LatentDiffusion(engine=RecEngine(), conditioning_key='hybrid', device_loop=True)      # hybrid c_concat
    hy.engine.set_concat = lambda cc: None
    per_step(hy, {'c_concat': [torch.rand(B, 5, H, W)], 'c_crossattn': [c]})
    per_step(_ldm(device_loop=True), {'c_concat': [torch.rand(B, 5, H, W)], 'c_crossattn': [c]})      # ... also where it is ignored
    per_step(_ldm(device_loop=True), [c, c])                                     # several c_crossattn parts
    per_step(_ldm(PerStepOnlyEngine(), device_loop=True), c)                     # an engine without the entry
    sp = _ldm(device_loop=True)                                                  # split_input_params: the patch branch of apply_model
    sp.split_input_params = {'ks': (4, 4), 'stride': (4, 4), 'clip_min_weight': 0.01, 'clip_max_weight': 0.5}
    sp.engine.apply_model_patches = lambda x, t, ctx, *a, **k: sp.engine.apply_model(x, t, ctx)
    per_step(sp, c)
    x0 = torch.randn(B, 4, H // 2, W)                                            # an x0 that is not the latent's shape
    bad = _ldm(device_loop=True)
    with pytest.raises(Exception):
        _loop(bad, c, x_T=x_T, timesteps=2, mask=torch.ones(1, 1, H // 2, 1), x0=x0)
    assert not bad.engine.ancestral
    clip = _ldm(device_loop=True, clip_denoised=True)                            # a refused option stays refused
    with pytest.raises(NotImplementedError):
        _loop(clip, c, x_T=x_T, timesteps=2)
    assert not clip.engine.ancestral
    # a ControlLDM with hints: the hint registered once, the scales handed over
    cm = models.ControlLDM(engine=RecEngine(n_controlnets=1), n_controlnets=1, device_loop=True)
    cm.control_scales = [0.5] * 13
    hint = torch.rand(B, 3, 8 * H, 8 * W)
    _loop(cm, {'c_concat': [hint], 'c_crossattn': [c]}, x_T=x_T, timesteps=3)
    k = cm.engine.ancestral[0]
    assert not cm.engine.calls and cm.engine.hints == [(0, hint)] and k['flags'] == 0 and list(k['control_scales']) == [0.5] * 13
    assert k['cond'] is c
    cm2 = models.ControlLDM(engine=RecEngine(n_controlnets=1), n_controlnets=1, device_loop=True)
    _loop(cm2, {'c_concat': None, 'c_crossattn': [c]}, x_T=x_T, timesteps=2)
    assert cm2.engine.ancestral[0]['flags'] == N and cm2.engine.ancestral[0]['control_scales'] is None


# ------------------------------------------------------------------------------------------------------------ noise order
@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('repeat', [False, True])
@pytest.mark.parametrize('bound', [256 << 20, 2 * B * 4 * H * W * 4])
def test_noise_is_drawn_in_the_per_step_order(draws, masked, repeat, bound):
    """per step p_sample's noise ((1, ...) under repeat_noise; also at t == 0), then q_sample's if there is a mask -- the same calls
    in the same order on both routes, however the walk is cut into segments -- and the same trajectory from the same seed"""
    x_T, c, _ = _inputs()
    S = 5
    kw = dict(x_T=x_T, timesteps=S, return_intermediates=True, log_every_t=2)
    if masked:
        kw.update(mask=(torch.arange(H) % 2 == 0).float().view(1, 1, H, 1), x0=torch.randn(B, 4, H, W, generator=torch.Generator().manual_seed(5)))
    if repeat:
        kw.update(repeat_noise=True)
    m2 = _ldm()
    ref, rinter = _loop(m2, c, **kw)
    per_step, after = list(draws), torch.randn(3)
    del draws[:]
    m = _ldm(device_loop=True)
    m.max_loop_noise_bytes = bound
    out, inter = _loop(m, c, **kw)
    assert torch.equal(after, torch.randn(3))                       # the generator is left where the per-step route leaves it
    one = [('randn', (1 if repeat else B, 4, H, W))] + ([('randn_like', (B, 4, H, W))] if masked else [])
    assert draws == per_step == one * S
    per = max(1, bound // (B * 4 * H * W * 4 * (2 if masked else 1)))
    assert len(m.engine.ancestral) == -(-S // per) and not m.engine.calls and not m2.engine.ancestral
    assert [t for k in m.engine.ancestral for t in k['timesteps']] == [4, 3, 2, 1, 0]
    assert all((k['q_noise'] is not None) == masked and tuple(k['step_noise'].shape[1:]) == (B, 4, H, W) for k in m.engine.ancestral)
    assert m.engine.evals == m2.engine.evals
    assert torch.equal(out, ref) and not torch.equal(out, x_T)
    assert len(inter) == len(rinter) == 4 and inter[0] is rinter[0]          # x_T, then t = 4, 2, 0
    assert all(torch.equal(a, b) for a, b in zip(inter, rinter))


def test_temperature_start_T_and_log_slots(draws):
    x_T, c, _ = _inputs()
    m, m2 = _ldm(device_loop=True), _ldm()
    kw = dict(x_T=x_T, timesteps=9, start_T=6, temperature=0.7, return_intermediates=True, log_every_t=4)
    out, inter = _loop(m, c, **kw)
    ref, rinter = _loop(m2, c, **kw)
    k = m.engine.ancestral[0]
    assert k['timesteps'] == [5, 4, 3, 2, 1, 0] and list(k['log_steps']) == [0, 1, 5]          # t = 5 (the first), 4 and 0
    h = m._host
    assert k['tables']['std'][:5] == [float(np.exp(0.5 * h['posterior_log_variance_clipped'][t])) * 0.7 for t in (5, 4, 3, 2, 1)]
    assert torch.equal(out, ref) and len(inter) == len(rinter) == 4 and all(torch.equal(a, b) for a, b in zip(inter, rinter))


# ------------------------------------------------------------------------------------------------------------ DDIM inversion
def _bits(v):
    return struct.pack('<f', v)


@pytest.mark.parametrize('original', [False, True])
def test_encode_tables_are_the_coefficients_the_per_step_encode_computed(draws, monkeypatch, original):
    """the formulas of the per-step encode as they stood before the helper (numpy float32 scalars, one step at a time), and what
    the per-step route now feeds to axpby"""
    x0, c, uc = _inputs()
    m = _ldm()
    s = samplers.ControlDDIMSampler(m)
    s.make_schedule(10, verbose=False)
    t_enc = 7
    if original:
        a_next = s.alphas_cumprod[:t_enc].detach().cpu().numpy().astype(np.float32)
        a_cur = s.alphas_cumprod_prev[:t_enc].detach().cpu().numpy().astype(np.float32)
    else:
        a_next = np.asarray(s.ddim_alphas[:t_enc], dtype=np.float32)
        a_cur = np.asarray(s.ddim_alphas_prev[:t_enc], dtype=np.float32)
    want = []
    for i in range(t_enc):
        f32 = np.float32
        cx = np.sqrt(a_next[i] / a_cur[i])
        ce = np.sqrt(a_next[i]) * (np.sqrt(f32(1) / a_next[i] - f32(1)) - np.sqrt(f32(1) / a_cur[i] - f32(1)))
        want.append((float(cx), float(ce)))
    cx, ce = samplers.encode_tables(a_next, a_cur)
    assert [(_bits(a), _bits(b)) for a, b in zip(cx, ce)] == [(_bits(a), _bits(b)) for a, b in want]
    assert all(isinstance(v, float) and float(np.float32(v)) == v for v in cx + ce)          # every entry is an fp32 value
    import types
    seen = []
    rec = types.SimpleNamespace(**{k: getattr(kernel_stubs, k) for k in dir(kernel_stubs) if not k.startswith('_')})
    rec.axpby = lambda a, ca, b, cb: (seen.append((ca, cb)), kernel_stubs.axpby(a, ca, b, cb))[1]
    monkeypatch.setattr(samplers, '_k', rec)
    s.encode(x0, c, t_enc, use_original_steps=original)
    assert [(_bits(a), _bits(b)) for a, b in seen] == [(_bits(a), _bits(b)) for a, b in want]
    # ... and the device route hands over the same tables
    m2 = _ldm()
    s2 = samplers.ControlDDIMSampler(m2, device_loop=True)
    s2.make_schedule(10, verbose=False)
    s2.encode(x0, c, t_enc, use_original_steps=original)
    k = m2.engine.encodes[0]
    assert [(_bits(a), _bits(b)) for a, b in zip(k['cx'], k['ce'])] == [(_bits(a), _bits(b)) for a, b in want]
    assert k['timesteps'] == ([0, 1, 2, 3, 4, 5, 6] if original else [int(t) for t in s2.ddim_timesteps[:t_enc]])


@pytest.mark.parametrize('scale,use_uc,ri', [(1.0, False, None), (3.0, True, None), (1.0, True, 2), (3.0, True, 2), (3.0, True, 5)])
def test_encode_routing_and_trajectory(draws, scale, use_uc, ri):
    x0, c, uc = _inputs()
    outs = []
    for loop in (False, True):
        m = _ldm()
        s = samplers.ControlDDIMSampler(m, device_loop=loop)
        s.make_schedule(8, verbose=False)
        outs.append((m, s.encode(x0, c, 5, return_intermediates=ri, unconditional_guidance_scale=scale,
                                 unconditional_conditioning=uc if use_uc else None)))
    (m2, (ref, rout)), (m, (out, dout)) = outs
    assert not m2.engine.encodes and len(m.engine.encodes) == 1 and not m.engine.calls
    k = m.engine.encodes[0]
    cfg_on = use_uc and scale != 1.0
    assert (k['uncond'] is uc) == cfg_on and k['flags'] == (N | _lib.FLAG_CFG_PAIRS if cfg_on else N) and k['cfg_scale'] == (scale if cfg_on else 1.0)
    assert k['log_steps'] == rout['intermediate_steps'] == dout['intermediate_steps']
    assert m.engine.evals == m2.engine.evals and len(m.engine.evals) == 5
    assert torch.equal(out, ref) and torch.equal(dout['x_encoded'], ref) and not torch.equal(out, x0)
    assert ('intermediates' in dout) == ('intermediates' in rout) == bool(ri)
    if ri:
        assert len(dout['intermediates']) == len(rout['intermediates']) == len(k['log_steps']) > 0
        assert all(torch.equal(a, b) for a, b in zip(dout['intermediates'], rout['intermediates']))


def test_encode_callback_and_missing_entry_keep_the_per_step_route(draws):
    x0, c, uc = _inputs()
    for eng, kw in ((RecEngine(), dict(callback=lambda i: None)), (PerStepOnlyEngine(), {})):
        m = _ldm(eng)
        s = samplers.ControlDDIMSampler(m, device_loop=True)
        s.make_schedule(8, verbose=False)
        s.encode(x0, c, 4, **kw)
        assert len(m.engine.calls) == 4 and not m.engine.encodes
    m = _ldm()
    s = samplers.ControlDDIMSampler(m)                        # off by default
    s.make_schedule(8, verbose=False)
    s.encode(x0, c, 4)
    assert s.device_loop is False and len(m.engine.calls) == 4 and not m.engine.encodes


# ------------------------------------------------------------------------------------------------------------ binding and header
def _header_struct(hdr, name):
    body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (name, name), hdr, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    return [re.sub(r'\s+', ' ', f).strip() for f in body.split(';') if f.strip()]


def _lib_or_build():
    if not os.path.exists(_lib.LIB_PATH):
        from fgdm_amd import build
        build.build(verbose=False)
    return _lib.load()


@pytest.mark.parametrize('name,cls_name,size,entry', [('fgdm_ancestral_params', 'FgdmAncestralParams', 176, 'fgdm_sample_ancestral'),
                                                      ('fgdm_ddim_encode_params', 'FgdmDdimEncodeParams', 112, 'fgdm_ddim_encode')])
def test_binding_header_and_library_declare_the_entries_and_the_same_structs(name, cls_name, size, entry):
    lib = _lib_or_build()
    assert getattr(lib, entry) is not None                                   # the built library exports the symbol
    cls = getattr(_lib, cls_name)
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
    # natural alignment, no hole and no tail padding: the offsets a C compiler gives the header's struct
    off = 0
    for fname, ftype in cls._fields_:
        assert getattr(cls, fname).offset == off and off % C.sizeof(ftype) == 0, fname
        off += C.sizeof(ftype)
    assert off == size and cls.struct_size.offset == 0 and cls.x.offset == 8 and cls.cond.offset == 16
    assert getattr(cls, 'reserved0').offset == size - (8 if name == 'fgdm_ancestral_params' else 4)
    assert 'fgdm_op_ancestral_loop_step' in _lib.SIGNATURES and 'fgdm_op_invert_loop_step' in _lib.SIGNATURES
    doc = re.sub(r'(\s|\*)+', ' ', hdr)
    for word in ('ddpm.py:1382-1448', 'ddpm.py:1419-1421', 'ddim_hacked.py:234-279', 'blend of the SAME step'):
        assert word in doc, word


def test_entries_refuse_bad_arguments_without_a_device():
    lib = _lib_or_build()
    for cls, fn in ((_lib.FgdmAncestralParams, lib.fgdm_sample_ancestral), (_lib.FgdmDdimEncodeParams, lib.fgdm_ddim_encode)):
        p = cls()
        p.struct_size = C.sizeof(p)
        assert fn(None, C.byref(p), None) == -1 and fn(None, None, None) == -1
    q, null = C.c_void_p(1 << 20), None
    anc = lambda x=q, eps=q, mask=null, x0=null, qn=null, n=64: \
        lib.fgdm_op_ancestral_loop_step(x, eps, 1.1, 0.4, 0.3, 0.7, 0.0, null, mask, x0, qn, 0.5, 0.5, q, null, null, n, null)
    assert anc(x=null) == -1 and anc(eps=null) == -1 and anc(n=0) == -1 and anc(n=-4) == -1
    assert anc(mask=q) == -1 and anc(mask=q, x0=q) == -1 and anc(mask=q, qn=q) == -1
    inv = lambda x=q, ec=q, n=64: lib.fgdm_op_invert_loop_step(x, ec, null, 1.0, 1.01, 0.02, q, null, null, null, n, null)
    assert inv(x=null) == -1 and inv(ec=null) == -1 and inv(n=0) == -1
