"""Host side of the device DDIM loop (fgdm_sample_ddim_ex), no GPU: the opt-in routing of DDIMSampler / ControlDDIMSampler with a
stub engine that records its calls -- which samplings are handed over, with which tables, and that the noise handed over is the
noise the per-step route draws from the same generator state -- plus the binding against include/fgdm.h."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

import kernel_stubs
from fgdm_amd import _lib, models, samplers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, H, W, TOK = 2, 8, 8, 77
N, O, P = _lib.FLAG_NO_CONTROL, _lib.FLAG_ONLY_MID_CONTROL, _lib.FLAG_CFG_PAIRS


class NoLoopEngine:
    """Records apply_model / set_hint (no GPU, no library); an engine without the device loop's entry."""
    has_vae, has_vae_encoder, has_clip = False, False, False
    device = torch.device('cpu')

    def __init__(self, n_controlnets=0):
        self.n_controlnets = n_controlnets
        self.calls, self.loops, self.hints = [], [], []

    def set_hint(self, cn, hint):
        self.hints.append((cn, hint))

    def apply_model(self, x, t, ctx, control_scales=None, flags=0, pcond=None, out=None):
        self.calls.append((tuple(x.shape), int(t[0]), tuple(ctx.shape), flags, None if control_scales is None else list(control_scales)))
        return 0.1 * x + 0.01 * ctx.mean()


class StubEngine(NoLoopEngine):
    """... and records sample_ddim_ex."""

    def sample_ddim_ex(self, x_T, cond, uncond, cfg_scale, timesteps, alphas, alphas_prev, sqrt_one_minus_alphas, **kw):
        self.loops.append(dict(kw, x_T=x_T, cond=cond, uncond=uncond, cfg_scale=cfg_scale, timesteps=list(timesteps),
                               alphas=np.asarray(alphas), alphas_prev=np.asarray(alphas_prev),
                               sqrt_one_minus_alphas=np.asarray(sqrt_one_minus_alphas)))
        n = len(kw.get('log_steps', ()))
        z = torch.zeros(n, *x_T.shape)
        return x_T.clone(), z, z.clone()


@pytest.fixture()
def stubs(monkeypatch):
    monkeypatch.setattr(samplers, '_k', kernel_stubs)
    monkeypatch.setattr(models, '_k', kernel_stubs)
    monkeypatch.setattr(samplers, '_randn', lambda shape, device: torch.randn(shape))
    monkeypatch.setattr(models, '_randn', lambda shape, device: torch.randn(shape))


def _inputs(seed=3):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return r(B, 4, H, W), r(B, TOK, 8), r(B, TOK, 8)


def _ldm():
    return models.LatentDiffusion(engine=StubEngine(), use_adapter=False)


def _cldm(**kw):
    return models.ControlLDM(engine=StubEngine(n_controlnets=1), n_controlnets=1, **kw)


def _run(sampler, cond, uc=None, scale=1.0, S=4, seed=11, **kw):
    torch.manual_seed(seed)
    return sampler.sample(S, B, (4, H, W), cond, verbose=False, unconditional_guidance_scale=scale,
                          unconditional_conditioning=uc, **kw)


def test_default_is_the_per_step_route_with_the_calls_of_before(stubs):
    x_T, c, uc = _inputs()
    for cls in (samplers.DDIMSampler, samplers.ControlDDIMSampler):
        m = _ldm()
        s = cls(m)
        assert s.device_loop is False
        out, inter = _run(s, c, uc, 7.5, x_T=x_T)
        assert not m.engine.loops
        ts = [int(t) for t in np.flip(s.ddim_timesteps)]
        assert m.engine.calls == [((2 * B, 4, H, W), t, (2 * B, TOK, 8), N | P, None) for t in ts]
        assert len(inter['x_inter']) == len(inter['pred_x0']) == 3          # x_T, the first step, the last step
    # ... and the default of the keyword: off
    m = _ldm()
    _run(samplers.DDIMSampler(m, device_loop=False), c, x_T=x_T)
    assert not m.engine.loops and len(m.engine.calls) == 4


def test_device_loop_hands_over_one_call_with_the_walk_tables(stubs):
    x_T, c, uc = _inputs()
    m = _ldm()
    s = samplers.DDIMSampler(m, device_loop=True)
    out, inter = _run(s, c, uc, 7.5, S=5, x_T=x_T, eta=0.7, temperature=0.8, log_every_t=200)
    assert not m.engine.calls and len(m.engine.loops) == 1
    k = m.engine.loops[0]
    assert k['timesteps'] == [int(t) for t in s.ddim_timesteps] and len(k['timesteps']) == 5       # ddim_timesteps order
    np.testing.assert_array_equal(k['alphas'], s.ddim_alphas)
    np.testing.assert_array_equal(k['alphas_prev'], s.ddim_alphas_prev)
    np.testing.assert_array_equal(k['sqrt_one_minus_alphas'], s.ddim_sqrt_one_minus_alphas)
    np.testing.assert_array_equal(k['sigmas'], s.ddim_sigmas)
    assert all(v != 0 for v in k['sigmas'])
    assert k['cond'] is c and k['uncond'] is uc and k['cfg_scales'] == [7.5] * 5 and k['flags'] == N | P
    assert k['control_scales'] is None and 'mask' not in k
    # index % 200 == 0 or index == S - 1 with index = S - 1 - i: the first and the last step of the walk
    assert list(k['log_steps']) == [0, 4]
    assert tuple(k['step_noise'].shape) == (5, B, 4, H, W)
    assert len(inter['x_inter']) == len(inter['pred_x0']) == 3 and inter['x_inter'][0] is x_T
    # CFG off: no unconditional half, no pair flag, no per-step scales
    for uc_, scale in ((None, 7.5), (uc, 1.0)):
        m = _ldm()
        _run(samplers.DDIMSampler(m, device_loop=True), c, uc_, scale, x_T=x_T)
        k = m.engine.loops[0]
        assert k['uncond'] is None and k['flags'] == N and k['cfg_scales'] is None and k['step_noise'] is None


def test_device_loop_tables_for_mask_decode_original_steps_and_control(stubs):
    x_T, c, uc = _inputs()
    x0 = torch.randn(B, 4, H, W, generator=torch.Generator().manual_seed(5))
    mask = (torch.arange(W) < W // 2).float().view(1, 1, 1, W)
    m = _ldm()
    s = samplers.DDIMSampler(m, device_loop=True)
    _run(s, c, uc, 5.0, x_T=x_T, mask=mask, x0=x0)
    k = m.engine.loops[0]
    assert tuple(k['mask'].shape) == (B, 4, H, W) and torch.equal(k['mask'], mask.expand(B, 4, H, W)) and k['x0'] is x0
    assert tuple(k['q_noise'].shape) == (4, B, 4, H, W) and k['step_noise'] is None          # eta = 0: drawn and dropped
    h = m._host
    assert k['sqrt_alphas_cumprod_t'] == [h['sqrt_alphas_cumprod'][t] for t in k['timesteps']]
    assert k['sqrt_one_minus_alphas_cumprod_t'] == [h['sqrt_one_minus_alphas_cumprod'][t] for t in k['timesteps']]
    # decode from t_start: the first t_start entries of the tables, no intermediates
    x = s.decode(x_T, c, 3, unconditional_guidance_scale=5.0, unconditional_conditioning=uc)
    k = m.engine.loops[1]
    assert k['timesteps'] == [int(t) for t in s.ddim_timesteps[:3]] and len(k['alphas']) == 3 and list(k['log_steps']) == []
    np.testing.assert_array_equal(k['alphas_prev'], s.ddim_alphas_prev[:3])
    assert torch.equal(x, x_T) and k['x_T'] is x_T
    # use_original_steps through ddim_sampling with timesteps=4: the model's own tables at t = 0 .. 3
    s.make_schedule(4, ddim_eta=0.5, verbose=False)
    torch.manual_seed(1)
    s.ddim_sampling(c, (B, 4, H, W), x_T=x_T, ddim_use_original_steps=True, timesteps=4, log_every_t=1)
    k = m.engine.loops[2]
    assert k['timesteps'] == [0, 1, 2, 3] and list(k['log_steps']) == [0, 1, 2, 3]
    np.testing.assert_array_equal(k['alphas'], m.alphas_cumprod.numpy()[:4])
    np.testing.assert_array_equal(k['sigmas'], s.ddim_sigmas_for_original_num_steps.numpy()[:4])
    assert k['sigmas'][0] == 0 and all(k['sigmas'][1:] > 0) and tuple(k['step_noise'].shape) == (4, B, 4, H, W)
    # ControlLDM: dict conds, the hint registered once, control scales, ucg_schedule as the per-step scales
    cm = _cldm(only_mid_control=True)
    cm.control_scales = [0.5] * 13
    hint = torch.rand(B, 3, 8 * H, 8 * W)
    cond, ucond = {'c_concat': [hint], 'c_crossattn': [c]}, {'c_concat': [hint], 'c_crossattn': [uc]}
    cs = samplers.ControlDDIMSampler(cm, device_loop=True)
    _run(cs, cond, ucond, 9.0, x_T=x_T, ucg_schedule=[9.0, 7.0, 5.0, 3.0])
    k = cm.engine.loops[0]
    assert not cm.engine.calls and cm.engine.hints == [(0, hint)] and cm.engine.hints[0][1] is hint
    assert k['cond'] is c and k['uncond'] is uc and k['cfg_scales'] == [9.0, 7.0, 5.0, 3.0] and k['flags'] == O | P
    assert list(k['control_scales']) == [0.5] * 13
    _run(cs, {'c_crossattn': [c], 'c_concat': None}, x_T=x_T)
    assert cm.engine.loops[1]['flags'] == O | N and cm.engine.loops[1]['control_scales'] is None


@pytest.mark.parametrize('eta,masked', [(0.0, False), (0.6, False), (0.0, True), (0.6, True)])
def test_device_loop_draws_the_noise_of_the_per_step_route(stubs, monkeypatch, eta, masked):
    """Same seed, both routes, x_T drawn too: the tensors handed to the device loop are, step by step, the q_sample noise and the
    step noise (times temperature) that the per-step route hands to its kernels."""
    _, c, uc = _inputs()
    x0 = torch.randn(B, 4, H, W, generator=torch.Generator().manual_seed(5))
    kw = dict(mask=(torch.arange(H) % 2 == 0).float().view(1, 1, H, 1), x0=x0) if masked else {}
    seen = {'q': [], 'step': []}
    real_axpby, real_step = kernel_stubs.axpby, kernel_stubs.ddim_step
    rec = types.SimpleNamespace(**{k: getattr(kernel_stubs, k) for k in dir(kernel_stubs) if not k.startswith('_')})
    rec.axpby = lambda a, ca, b, cb: (seen['q'].append(b), real_axpby(a, ca, b, cb))[1]
    rec.ddim_step = lambda x, ec, eu, s, a, ap, sig, s1m, noise=None, want=True: (seen['step'].append(noise), real_step(x, ec, eu, s, a, ap, sig, s1m, noise, want))[1]
    monkeypatch.setattr(samplers, '_k', rec)
    monkeypatch.setattr(models, '_k', rec)
    m = _ldm()
    out, inter = _run(samplers.DDIMSampler(m), c, uc, 7.5, S=4, eta=eta, temperature=0.8, **kw)
    m2 = _ldm()
    _run(samplers.DDIMSampler(m2, device_loop=True), c, uc, 7.5, S=4, eta=eta, temperature=0.8, **kw)
    k = m2.engine.loops[0]
    assert torch.equal(k['x_T'], inter['x_inter'][0])                        # the same x_T came first
    assert len(seen['step']) == 4 and len(seen['q']) == (4 if masked else 0)
    if eta:
        assert all(torch.equal(k['step_noise'][i], seen['step'][i]) for i in range(4))
    else:
        assert k['step_noise'] is None and all(v is None for v in seen['step'])
    if masked:
        assert all(torch.equal(k['q_noise'][i], seen['q'][i]) for i in range(4))
    # ... and the generator ends where the per-step route leaves it
    a = torch.randn(3)
    _run(samplers.DDIMSampler(_ldm()), c, uc, 7.5, S=4, eta=eta, temperature=0.8, **kw)
    assert torch.equal(a, torch.randn(3))


def test_everything_out_of_scope_takes_the_per_step_route(stubs):
    x_T, c, uc = _inputs()

    def per_step(model=None, cond=c, ucond=uc, cls=samplers.DDIMSampler, calls=4, **kw):
        m = model or _ldm()
        _run(cls(m, device_loop=True), cond, ucond, 7.5, x_T=x_T, **kw)
        assert not m.engine.loops and len(m.engine.calls) == calls, kw

    per_step(callback=lambda i: None)
    per_step(img_callback=lambda p, i: None)
    per_step(noise_dropout=0.1, eta=0.5)
    per_step(augmented_conditoning=True, ac=c.clone())
    # composable_diffusion (ddim.py:204-212): a batch of n + 1 rows of ONE sample, so a batch of one
    m = _ldm()
    torch.manual_seed(11)
    samplers.DDIMSampler(m, device_loop=True).sample(4, 1, (4, H, W), c[:1].clone(), verbose=False, x_T=x_T[:1].clone(),
                                                     unconditional_guidance_scale=7.5, unconditional_conditioning=uc[:1].clone(),
                                                     composable_diffusion=1)
    assert not m.engine.loops and [k[0] for k in m.engine.calls] == [(2, 4, H, W)] * 4
    # (repeat_noise, the remaining option of p_sample_ddim, is no keyword of sample(), ddim_sampling() or decode() and is not
    # forwarded by them: it cannot reach the routing)
    import inspect
    for fn in (samplers.DDIMSampler.sample, samplers.DDIMSampler.ddim_sampling, samplers.DDIMSampler.decode,
               samplers.ControlDDIMSampler.sample, samplers.ControlDDIMSampler.ddim_sampling):
        assert 'repeat_noise' not in inspect.signature(fn).parameters
    # a plain DDIMSampler on a ControlLDM with dict conds under CFG: its torch.cat of two dicts fails as it did, no loop
    cm0 = _cldm()
    with pytest.raises(TypeError):
        _run(samplers.DDIMSampler(cm0, device_loop=True), {'c_crossattn': [c], 'c_concat': None},
             {'c_crossattn': [uc], 'c_concat': None}, 7.5, x_T=x_T)
    assert not cm0.engine.loops
    # a ControlLDM subclass with an apply_model of its own is not bypassed

    class OwnApply(models.ControlLDM):
        def apply_model(self, x_noisy, t, cond, *args, **kwargs):
            return super().apply_model(x_noisy, t, cond, *args, **kwargs)
    own = OwnApply(engine=StubEngine(n_controlnets=1), n_controlnets=1)
    per_step(model=own, cond={'c_crossattn': [c], 'c_concat': None}, ucond={'c_crossattn': [uc], 'c_concat': None},
             cls=samplers.ControlDDIMSampler)
    per_step(use_original=True)                                     # any kwarg the per-step route forwards to apply_model

    class Corrector:
        def modify_score(self, model, e, x, t, c):
            return e
    per_step(score_corrector=Corrector())
    per_step(cond={'c_crossattn': [c]}, ucond=None)                 # a dict cond on a model that is no ControlLDM
    # ucg_schedule that is 1 at some steps: those steps run without the unconditional half
    cm = _cldm()
    cond, ucond = {'c_crossattn': [c], 'c_concat': None}, {'c_crossattn': [uc], 'c_concat': None}
    per_step(model=cm, cond=cond, ucond=ucond, cls=samplers.ControlDDIMSampler, ucg_schedule=[7.5, 1.0, 7.5, 1.0])
    # branches with different hints: two calls per step
    hint = torch.rand(B, 3, 8 * H, 8 * W)
    per_step(model=_cldm(), cond={'c_concat': [hint], 'c_crossattn': [c]}, ucond=ucond, cls=samplers.ControlDDIMSampler, calls=8)
    # hybrid c_concat
    hy = models.LatentDiffusion(engine=StubEngine(), conditioning_key='hybrid')
    hy.engine.set_concat = lambda cc: None
    cc = torch.rand(B, 5, H, W)
    per_step(model=hy, cls=samplers.ControlDDIMSampler, cond={'c_concat': [cc], 'c_crossattn': [c]},
             ucond={'c_concat': [cc], 'c_crossattn': [uc]})
    # split_input_params: LatentDiffusion.apply_model's patch branch
    sp = _ldm()
    sp.split_input_params = {'ks': (4, 4), 'stride': (4, 4), 'clip_min_weight': 0.01, 'clip_max_weight': 0.5}
    sp.engine.apply_model_patches = lambda x, t, ctx, *a, **k: sp.engine.apply_model(x, t, ctx)
    per_step(model=sp)
    # an engine without the entry, and a model without an engine
    per_step(model=models.LatentDiffusion(engine=NoLoopEngine(), use_adapter=False))

    class Bare:
        num_timesteps = 1000
        parameterization = 'eps'
        device = 'cpu'

        def __init__(self):
            ref = _ldm()
            self.betas, self.alphas_cumprod, self.alphas_cumprod_prev = ref.betas, ref.alphas_cumprod, ref.alphas_cumprod_prev
            self.calls = 0

        def apply_model(self, x, t, c, **kw):
            self.calls += 1
            return 0.1 * x
    bare = Bare()
    _run(samplers.DDIMSampler(bare, device_loop=True), c, uc, 7.5, x_T=x_T)
    assert bare.calls == 4
    # decode: a callback, and a ucg_schedule left over from ControlDDIMSampler.ddim_sampling
    m = _ldm()
    s = samplers.DDIMSampler(m, device_loop=True)
    s.make_schedule(4, verbose=False)
    s.decode(x_T, c, 3, callback=lambda i: None)
    assert not m.engine.loops and len(m.engine.calls) == 3
    cm = _cldm()
    cs = samplers.ControlDDIMSampler(cm, device_loop=True)
    _run(cs, cond, ucond, 7.5, x_T=x_T, ucg_schedule=[7.5, 6.0, 5.0, 4.0])
    assert len(cm.engine.loops) == 1
    cs.decode(x_T, cond, 2, unconditional_guidance_scale=7.5, unconditional_conditioning=ucond)
    assert len(cm.engine.loops) == 1 and len(cm.engine.calls) == 2


def test_refusals_still_raise(stubs):
    x_T, c, uc = _inputs()
    for kw in (dict(quantize_x0=True), dict(inference_loss=True), dict(return_conds=True)):
        m = _ldm()
        with pytest.raises(NotImplementedError):
            _run(samplers.DDIMSampler(m, device_loop=True), c, uc, 7.5, x_T=x_T, **kw)
        assert not m.engine.loops
    cm = _cldm()
    with pytest.raises(NotImplementedError):
        _run(samplers.ControlDDIMSampler(cm, device_loop=True), {'c_crossattn': [c], 'c_concat': None}, x_T=x_T, dynamic_threshold=0.9)
    assert not cm.engine.loops


# ------------------------------------------------------------------------------------------------------------ binding and header
def test_binding_and_header_declare_the_entry_and_the_same_struct():
    assert 'fgdm_sample_ddim_ex' in _lib.SIGNATURES and 'fgdm_op_ddim_loop_step' in _lib.SIGNATURES
    res, args = _lib.SIGNATURES['fgdm_sample_ddim_ex']
    assert res is C.c_int and args[1]._type_ is _lib.FgdmDdimParams
    hdr = open(os.path.join(ROOT, 'include', 'fgdm.h')).read()
    assert re.search(r'\bint\s+fgdm_sample_ddim_ex\s*\(\s*fgdm_engine\*\s*e,\s*const fgdm_ddim_params\*\s*p,\s*void\*\s*stream\)\s*;', hdr)
    body = re.search(r'typedef struct fgdm_ddim_params \{(.*?)\} fgdm_ddim_params;', hdr, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = [re.sub(r'\s+', ' ', f).strip() for f in body.split(';') if f.strip()]
    kind = lambda decl: 'ptr' if '*' in decl else decl.rsplit(' ', 1)[0]
    want = {'ptr': C.c_void_p, 'int64_t': C.c_int64, 'int32_t': C.c_int32, 'float': C.c_float}
    got = _lib.FgdmDdimParams._fields_
    assert [f.rsplit(' ', 1)[1].lstrip('*') for f in fields] == [n for n, _ in got]
    assert [want[kind(f)] for f in fields] == [t for _, t in got]
    assert fields[0] == 'int64_t struct_size' and C.sizeof(_lib.FgdmDdimParams) == 192
    assert int(re.search(r'#define FGDM_DDIM_PARAMS_SIZE_V1 (\d+)', hdr).group(1)) == 192      # the first version: this struct
    doc = re.sub(r'(\s|\*)+', ' ', hdr[:hdr.index('typedef struct fgdm_ddim_params')])
    for word in ('ddim.py:151-154', 'ddim_hacked.py:159-161', 'WALK order', 'struct_size', 'FGDM_ERR_ARG before any launch'):
        assert word in doc, word


def test_entries_refuse_null_arguments_without_a_device():
    if not os.path.exists(_lib.LIB_PATH):
        from fgdm_amd import build
        build.build(verbose=False)
    lib = _lib.load()
    p = _lib.FgdmDdimParams()
    p.struct_size = C.sizeof(p)
    assert lib.fgdm_sample_ddim_ex(None, C.byref(p), None) == -1 and lib.fgdm_sample_ddim_ex(None, None, None) == -1
    q, null = C.c_void_p(1 << 20), None
    step = lambda x=q, ec=q, eu=null, mask=null, x0=null, qn=null, n=64: lib.fgdm_op_ddim_loop_step(
        x, ec, eu, 1.0, 0.5, 0.6, 0.0, 0.7, null, mask, x0, qn, 0.5, 0.5, q, null, null, null, null, n, null)
    assert step(x=null) == -1 and step(n=0) == -1 and step(ec=null, eu=q) == -1
    assert step(mask=q) == -1 and step(mask=q, x0=q) == -1 and step(mask=q, qn=q) == -1


def test_converted_tensors_live_until_the_native_call_returns():
    """a step tensor that is not fp32, contiguous and on the engine's device is copied; the struct must point into a copy that is
    still alive while the native loop runs, and a log plane allocated afterwards must not land in a freed copy"""
    from fgdm_amd import engine as E

    class HostEngine(E.Engine):
        def __init__(self):
            self.device, self.seen = torch.device('cpu'), None

        def set_context_tokens(self, n):
            pass

        def _run_loop(self, name, p, keep, control_scales, call=None):
            self.seen = (p, {t.data_ptr() for t in keep if torch.is_tensor(t)})

    e, S = HostEngine(), 3
    x, c = torch.randn(1, 4, 8, 8), torch.randn(1, 77, 8)
    noise = torch.randn(S, 1, 4, 8, 8, dtype=torch.float64)                       # another dtype
    mask = torch.ones(1, 4, 8, 8).transpose(2, 3)                                  # not contiguous
    tab = [0.5] * S
    for call in (lambda: e.sample_ddim_ex(x, c, None, 1.0, [1, 2, 3], tab, tab, tab, sigmas=tab, step_noise=noise, mask=mask, x0=x.double(),
                                          q_noise=noise, sqrt_alphas_cumprod_t=tab, sqrt_one_minus_alphas_cumprod_t=tab, log_steps=(1,)),
                 lambda: e.sample_plms(x, c, None, 1.0, [1, 2, 3], tab, tab, tab, mask=mask, x0=x.double(), q_noise=noise,
                                       sqrt_alphas_cumprod_t=tab, sqrt_one_minus_alphas_cumprod_t=tab, log_steps=(1,)),
                 lambda: e.sample_ancestral(x, c, [3, 2, 1], dict(sqrt_recip_alphas_cumprod=tab, sqrt_recipm1_alphas_cumprod=tab,
                                                                  posterior_mean_coef1=tab, posterior_mean_coef2=tab, std=tab,
                                                                  sqrt_alphas_cumprod_t=tab, sqrt_one_minus_alphas_cumprod_t=tab),
                                            step_noise=noise, mask=mask, x0=x.double(), q_noise=noise, log_steps=(1,))):
        call()
        p, alive = e.seen
        fields = [k for k in ('step_noise', 'q_noise', 'mask', 'x0') if hasattr(p, k)]
        assert len(fields) >= 3
        for k in fields:
            assert getattr(p, k) in alive, k
        assert p.mask != mask.data_ptr() and p.q_noise != noise.data_ptr()
        assert p.x_inter_out and p.x_inter_out not in alive
