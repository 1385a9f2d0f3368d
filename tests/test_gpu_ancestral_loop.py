"""The device ancestral loop and the device DDIM inversion (fgdm_sample_ancestral / k_ancestral_loop_step, fgdm_ddim_encode /
k_invert_loop_step) on the GPU.

The yardstick is torch.equal.  The step kernels alone (fgdm_op_ancestral_loop_step, fgdm_op_invert_loop_step) against the chain of
existing kernels each launch fuses (tests/ancestral_loops.py: ancestral_step -> axpby + mask_blend; cfg_combine -> axpby), on
inputs whose dynamic range makes a contracted or a split fma visible, every output poisoned and guarded (tests/guarded.py).  Then
LatentDiffusion / ControlLDM(device_loop=True).p_sample_loop and ControlDDIMSampler(device_loop=True).encode against the per-step
route on the same engine from the same generator state: same networks, same arithmetic rounding for rounding, so there is no
tolerance -- and the per-step routes are the ones tests/test_gpu_samplers.py holds to the reference.

The reduced synthetic engine (golden_inputs.SMALL_CFG, one ControlNet) at 8 x 8 latents."""
import ctypes as C

import pytest
import torch

import ancestral_loops as al
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
    """every sample_ancestral / ddim_encode of the test runs on guarded buffers, checked when the call returns"""
    real = {'sample_ancestral': engine.sample_ancestral, 'ddim_encode': engine.ddim_encode}
    runs = []

    def wrap(name):
        def call(x, *a, **k):
            n_log = len(k.get('log_steps', ()))
            gx = guarded_out(tuple(x.shape), torch.float32)
            gl = guarded_out((n_log, *x.shape), torch.float32) if n_log else None
            out = real[name](x, *a, **k, out=gx.t, x_inter_out=gl and gl.t)
            torch.cuda.synchronize()
            gx.check()
            if gl is not None:
                gl.check()
            runs.append((name, n_log))
            return out
        return call
    for name in real:
        monkeypatch.setattr(engine, name, wrap(name))
    return runs


def _ldm(engine, loop):
    from fgdm_amd import models
    return models.LatentDiffusion(gi.SMALL_CFG, engine=engine, use_adapter=False, device_loop=loop)


def _cldm(engine, loop):
    from fgdm_amd import models
    m = models.ControlLDM(gi.SMALL_CFG, engine=engine, n_controlnets=1, device_loop=loop)
    m.control_scales = [0.9] * 13
    return m


def _inputs(B=2, H=8, W=8, seed=900):
    x = torch.from_numpy(synth.latents(B, H, W, seed=seed)).cuda()
    c = torch.from_numpy(synth.context(B, seed=seed + 1)).cuda()
    uc = torch.from_numpy(synth.context(B, seed=seed + 2)).cuda()
    return x, c, uc


def _half_mask(H, W):
    return (torch.arange(W) < W // 2).float().view(1, 1, 1, W).expand(1, 1, H, W).cuda()


def _both(run, seed=1234):
    """run(device_loop) on the per-step route, then on the device route, from the same generator state"""
    outs = []
    for loop in (False, True):
        torch.manual_seed(seed)
        outs.append(run(loop))
    return outs


# ------------------------------------------------------------------------------------------------------------ the ancestral walk
# p_sample_loop's keywords (S = 6 steps), logged latents behind x_T
WALKS = {
    'plain': (dict(), None),
    'mask': (dict(mask='half'), None),
    'temperature': (dict(temperature=0.7), None),
    'repeat_noise': (dict(repeat_noise=True), None),
    'start_T': (dict(timesteps=9, start_T=6), None),
    'intermediates': (dict(return_intermediates=True, log_every_t=4), 3),           # t = 5 (the first step), 4 and 0
    'mask_intermediates': (dict(mask='half', return_intermediates=True, log_every_t=3), 3),      # t = 5, 3, 0, after the blend
}


def _walk_kw(name, B, H=8, W=8):
    kw, n_logged = WALKS[name]
    kw = dict(kw)
    kw.setdefault('timesteps', 6)
    if kw.pop('mask', None):
        kw['x0'] = torch.from_numpy(synth.latents(B, H, W, seed=911)).cuda()
        kw['mask'] = _half_mask(H, W)
    return kw, n_logged


def _same_walk(a, b, n_logged):
    if n_logged is None:
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())
        return a
    (xa, ia), (xb, ib) = a, b
    assert torch.equal(xa, xb) and bool(torch.isfinite(xa).all())
    assert len(ia) == len(ib) == n_logged + 1
    for j, (u, v) in enumerate(zip(ia, ib)):
        assert torch.equal(u, v), j
    assert torch.equal(ib[-1], xb)              # t = 0 is logged: the sample itself, after its blend
    return xa


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('name', list(WALKS))
def test_device_walk_equals_per_step_route(engine, guard, name, B):
    kw, n_logged = _walk_kw(name, B)
    x_T, c, _ = _inputs(B)
    a, b = _both(lambda loop: _ldm(engine, loop).p_sample_loop(c, (B, 4, 8, 8), x_T=x_T, **kw))
    out = _same_walk(a, b, n_logged)
    assert guard == [('sample_ancestral', n_logged or 0)], 'the device loop did not take this walk over'
    assert not torch.equal(out, x_T)


def test_sample_draws_x_T_and_takes_the_device_route(engine, guard):
    _, c, _ = _inputs(2)
    a, b = _both(lambda loop: _ldm(engine, loop).sample(c, batch_size=2, timesteps=3, shape=(2, 4, 8, 8)))
    assert torch.equal(a, b) and guard == [('sample_ancestral', 0)]


@pytest.mark.parametrize('name', ['plain', 'mask_intermediates', 'repeat_noise'])
def test_three_segments_give_the_bits_of_one(engine, guard, name):
    B = 3
    kw, n_logged = _walk_kw(name, B)
    x_T, c, _ = _inputs(B)
    step = B * 4 * 8 * 8 * 4 * (2 if 'mask' in kw else 1)

    def run(bound):
        m = _ldm(engine, True)
        m.max_loop_noise_bytes = bound
        torch.manual_seed(77)
        return m.p_sample_loop(c, (B, 4, 8, 8), x_T=x_T, **kw)
    one = run(256 << 20)
    assert [r[0] for r in guard] == ['sample_ancestral']
    three = run(2 * step + 5)                   # two steps fit, a third does not: 6 steps in three calls
    assert len(guard) == 4
    _same_walk(one, three, n_logged)
    if n_logged is not None:
        assert sum(r[1] for r in guard[1:]) == n_logged


def test_control_ldm_with_hints_and_scales(engine, guard):
    x_T, c, _ = _inputs()
    hint = torch.from_numpy(synth.hint(2, res=64, seed=903)).cuda()
    run = lambda loop, h=hint: _cldm(engine, loop).p_sample_loop({'c_concat': [h], 'c_crossattn': [c]}, (2, 4, 8, 8), x_T=x_T, timesteps=6)
    a, b = _both(run)
    assert torch.equal(a, b) and guard == [('sample_ancestral', 0)]
    torch.manual_seed(1234)                                      # ... and the hint matters
    assert not torch.equal(run(True, hint.flip(-1).contiguous()), a)


# ------------------------------------------------------------------------------------------------------------ DDIM inversion
ENCODES = {
    'cfg_off': dict(),
    'cfg_on': dict(unconditional_guidance_scale=3.0, uc=True),
    'original_steps': dict(use_original_steps=True, unconditional_guidance_scale=3.0, uc=True),
    'intermediates': dict(return_intermediates=2, unconditional_guidance_scale=3.0, uc=True),
    'intermediates_cfg_off': dict(return_intermediates=2),
}


@pytest.mark.parametrize('name', list(ENCODES))
def test_device_encode_equals_per_step_route(engine, guard, name):
    from fgdm_amd import samplers
    kw = dict(ENCODES[name])
    x0, c, uc = _inputs()
    if kw.pop('uc', False):
        kw['unconditional_conditioning'] = uc

    def run(loop):
        s = samplers.ControlDDIMSampler(_ldm(engine, False), device_loop=loop)
        s.make_schedule(10, verbose=False)
        return s.encode(x0, c, 5, **kw)
    (xa, oa), (xb, ob) = _both(run)
    assert torch.equal(xa, xb) and torch.equal(ob['x_encoded'], xa) and bool(torch.isfinite(xa).all()) and not torch.equal(xa, x0)
    assert oa['intermediate_steps'] == ob['intermediate_steps']
    n_log = len(oa['intermediate_steps'])
    assert guard == [('ddim_encode', n_log)], 'the device loop did not take this inversion over'
    if kw.get('return_intermediates'):
        assert oa['intermediate_steps'] == [0, 2, 3, 4] and len(oa['intermediates']) == len(ob['intermediates']) == 4
        for j, (u, v) in enumerate(zip(oa['intermediates'], ob['intermediates'])):
            assert torch.equal(u, v), j
    else:
        assert 'intermediates' not in ob and n_log == 0


def test_control_ldm_encode_with_hint_and_cfg(engine, guard):
    from fgdm_amd import samplers
    x0, c, uc = _inputs()
    hint = torch.from_numpy(synth.hint(2, res=64, seed=903)).cuda()
    cond, ucond = {'c_concat': [hint], 'c_crossattn': [c]}, {'c_concat': [hint], 'c_crossattn': [uc]}

    def run(loop):
        s = samplers.ControlDDIMSampler(_cldm(engine, False), device_loop=loop)
        s.make_schedule(10, verbose=False)
        return s.encode(x0, cond, 5, unconditional_guidance_scale=3.0, unconditional_conditioning=ucond)[0]
    a, b = _both(run)
    assert torch.equal(a, b) and guard == [('ddim_encode', 0)] and not torch.equal(a, x0)


# ------------------------------------------------------------------------------------------------------------ the kernels alone
def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def ancestral_op(lib, null=()):
    """ancestral_loops' step() as ONE launch of fgdm_op_ancestral_loop_step on poisoned, guarded outputs.  null: outputs handed
    over as NULL."""
    def step(x, eps, coef, noise, blend):
        outs = {k: None if k in null else guarded_out(tuple(x.shape), torch.float32) for k in ('x_out', 'xin', 'log_x')}
        mask, x0, qn, sa, s1m = blend if blend is not None else (None, None, None, 0.0, 0.0)
        ptr = lambda k: _p(outs[k] and outs[k].t)
        rc = lib.fgdm_op_ancestral_loop_step(_p(x), _p(eps), *coef, _p(noise), _p(mask), _p(x0), _p(qn), sa, s1m, ptr('x_out'),
                                             ptr('xin'), ptr('log_x'), x.numel(), None)
        torch.cuda.synchronize()
        assert rc == 0
        return {k: None if g is None else g.check() for k, g in outs.items()}
    return step


def invert_op(lib, null=()):
    def step(x, ec, eu, cfg, cx, ce):
        outs = {k: None if k in null else guarded_out(tuple(x.shape), torch.float32) for k in ('x_out', 'xin_a', 'xin_b', 'log_x')}
        ptr = lambda k: _p(outs[k] and outs[k].t)
        rc = lib.fgdm_op_invert_loop_step(_p(x), _p(ec), _p(eu), cfg, cx, ce, ptr('x_out'), ptr('xin_a'), ptr('xin_b'), ptr('log_x'),
                                          x.numel(), None)
        torch.cuda.synchronize()
        assert rc == 0
        return {k: None if g is None else g.check() for k, g in outs.items()}
    return step


def _wide(n, g, scale_lo=-2.0, scale_hi=4.0):
    """randn times 10 ** U(lo, hi): magnitudes from 1e-2 up to 1e4 side by side"""
    return torch.randn(n, generator=g) * 10.0 ** (scale_lo + (scale_hi - scale_lo) * torch.rand(n, generator=g))


# a single element, less than one block, a tail behind 1024 blocks; 4096 * 256 + 77: a second grid-stride pass (the grid is
# capped at 4096 blocks of 256), the size of the sibling loops' step-kernel tests
SIZES = [1, 255, 256 * 1024 + 3, 4096 * 256 + 77]


def _all_equal(got, want, what):
    for k, v in got.items():
        assert v is None or torch.equal(v, want), (what, k)


@pytest.mark.parametrize('n', SIZES)
def test_ancestral_step_kernel_equals_the_kernels_it_fuses(n):
    from fgdm_amd import _lib, engine as E
    lib = _lib.load()
    g = torch.Generator().manual_seed(n)
    x = guarded_in(torch.randn(n, generator=g) * 1e-3)                                  # x near 0 against |eps| up to 1e4
    eps, noise = (guarded_in(_wide(n, g)) for _ in range(2))
    x0, qn = (guarded_in(torch.randn(n, generator=g)) for _ in range(2))
    mask = (torch.rand(n, generator=g) < 0.5).float()
    mask[::7] = 0.3                                                                      # 0 / 1 and soft values
    mask = guarded_in(mask)
    # coefficients of the size the schedule holds at a middle timestep, none of them a power of two
    coef, sa, s1m = (1.5719, 1.2128, 0.0127, 0.9871, 0.0631), 0.6362, 0.7715
    chain = al.ancestral_chain(E)
    blend = (mask, x0, qn, sa, s1m)
    seen = []
    for bl in (blend, None):
        for nz, cf in ((noise, coef), (None, coef), (noise, coef[:4] + (0.0,))):        # noise NULL and std == 0: the t == 0 step
            want = chain(x, eps, cf, nz, bl)
            seen.append(want)
            what = (bl is not None, nz is not None, cf[4])
            _all_equal(ancestral_op(lib)(x, eps, cf, nz, bl), want, what)
            for off in ('x_out', 'xin', 'log_x'):                                        # every optional output NULL in turn
                got = ancestral_op(lib, null=(off,))(x, eps, cf, nz, bl)
                assert got[off] is None
                _all_equal(got, want, what + (off,))
    if n > 1:
        assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[0], seen[3]) and torch.equal(seen[1], seen[2])
    # in place, as the loop runs it: x_out is the state
    want = chain(x, eps, coef, noise, blend)
    state, xin = guarded_out((n,), torch.float32), guarded_out((n,), torch.float32)
    state.t.copy_(x)
    rc = lib.fgdm_op_ancestral_loop_step(_p(state.t), _p(eps), *coef, _p(noise), _p(mask), _p(x0), _p(qn), sa, s1m, _p(state.t),
                                         _p(xin.t), None, n, None)
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(state.check(), want) and torch.equal(xin.check(), want)


@pytest.mark.parametrize('n', SIZES)
def test_invert_step_kernel_equals_the_kernels_it_fuses(n):
    from fgdm_amd import _lib, engine as E
    lib = _lib.load()
    g = torch.Generator().manual_seed(n + 1)
    x = guarded_in(torch.randn(n, generator=g) * 1e-3)
    ec, eu = (guarded_in(_wide(n, g)) for _ in range(2))
    cfg, cx, ce = 3.0, 1.0213, 0.0347
    chain = al.invert_chain(E)
    for u in (eu, None):
        want = chain(x, ec, u, cfg, cx, ce)
        _all_equal(invert_op(lib)(x, ec, u, cfg, cx, ce), want, u is not None)
        for off in ('x_out', 'xin_a', 'xin_b', 'log_x'):
            got = invert_op(lib, null=(off,))(x, ec, u, cfg, cx, ce)
            assert got[off] is None
            _all_equal(got, want, (u is not None, off))
    if n > 1:
        assert not torch.equal(chain(x, ec, eu, cfg, cx, ce), chain(x, ec, None, cfg, cx, ce))
    want = chain(x, ec, eu, cfg, cx, ce)
    state, half = guarded_out((n,), torch.float32), guarded_out((n,), torch.float32)
    state.t.copy_(x)
    rc = lib.fgdm_op_invert_loop_step(_p(state.t), _p(ec), _p(eu), cfg, cx, ce, _p(state.t), None, _p(half.t), None, n, None)
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(state.check(), want) and torch.equal(half.check(), want)


# ------------------------------------------------------------------------------------------------------------ argument errors
def _arr(keep, v, ty=C.c_float):
    keep.append((ty * len(v))(*[ty(x).value for x in v]))
    return C.cast(keep[-1], C.c_void_p)


S_ARG = 4


def _ancestral_params(x_, c_, uc_, **over):
    from fgdm_amd import _lib
    keep = []
    p = _lib.FgdmAncestralParams()
    p.struct_size = C.sizeof(p)
    p.x, p.cond = x_.data_ptr(), c_.data_ptr()
    p.timesteps = _arr(keep, [3, 2, 1, 0], C.c_int64)
    p.sqrt_recip_alphas_cumprod, p.sqrt_recipm1_alphas_cumprod = _arr(keep, [1.003] * S_ARG), _arr(keep, [0.07] * S_ARG)
    p.posterior_mean_coef1, p.posterior_mean_coef2 = _arr(keep, [0.4] * S_ARG), _arr(keep, [0.6] * S_ARG)
    p.std = _arr(keep, [0.0] * S_ARG)
    p.S, p.B, p.H, p.W, p.flags = S_ARG, x_.shape[0], x_.shape[2], x_.shape[3], _lib.FLAG_NO_CONTROL
    for k, v in over.items():
        setattr(p, k, _arr(keep, *v) if isinstance(v, tuple) else v)
    return p, keep


def _encode_params(x_, c_, uc_, **over):
    from fgdm_amd import _lib
    keep = []
    p = _lib.FgdmDdimEncodeParams()
    p.struct_size = C.sizeof(p)
    p.x, p.cond, p.uncond = x_.data_ptr(), c_.data_ptr(), uc_.data_ptr()
    p.timesteps = _arr(keep, [1, 101, 201, 301], C.c_int64)
    p.cx, p.ce = _arr(keep, [1.02] * S_ARG), _arr(keep, [0.03] * S_ARG)
    p.cfg_scale, p.S, p.B, p.H, p.W, p.flags = 3.0, S_ARG, x_.shape[0], x_.shape[2], x_.shape[3], _lib.FLAG_NO_CONTROL
    for k, v in over.items():
        setattr(p, k, _arr(keep, *v) if isinstance(v, tuple) else v)
    return p, keep


def _levels(engine):
    st = engine.workspace_stats()
    return st['peak_bytes'], st['reserved_bytes']


def _refused(engine, entry, make, bad, x0, c, uc, out):
    """every case returns FGDM_ERR_ARG before any launch: x and the log plane untouched, the workspace at its level"""
    before = _levels(engine)
    for why, over in bad.items():
        x = guarded_out(tuple(x0.shape), torch.float32)
        x.t.copy_(x0)
        p, keep = make(x.t, c, uc, **over)
        rc = getattr(engine.lib, entry)(engine.h, C.byref(p), None)
        torch.cuda.synchronize()
        assert rc == ERR_ARG, why
        assert torch.equal(x.t, x0), why
        x.check_guards()
        out.check_guards()
        out.assert_untouched((slice(None),))
        assert entry.encode() in engine.lib.fgdm_last_error(engine.h), why
        assert _levels(engine) == before, why


def _log_cases(out):
    i32 = C.c_int32
    return {
        'log step out of range': dict(n_log=2, log_steps=([0, 4], i32), x_inter_out=out.t.data_ptr()),
        'log step negative': dict(n_log=1, log_steps=([-1], i32), x_inter_out=out.t.data_ptr()),
        'log steps not ascending': dict(n_log=2, log_steps=([1, 1], i32), x_inter_out=out.t.data_ptr()),
        'log steps missing': dict(n_log=1, x_inter_out=out.t.data_ptr()),
        'negative n_log': dict(n_log=-1),
        'reserved0 set': dict(reserved0=1),
        'x NULL': dict(x=None),
        'cond NULL': dict(cond=None),
        'timesteps NULL': dict(timesteps=None),
        'no steps': dict(S=0),
        'B = 0': dict(B=0),
        'H < 0': dict(H=-8),
        'W = 0': dict(W=0),
    }


def _runs_and_returns_its_workspace(engine, entry, make, x0, c, uc, out):
    """the same parameters without a defect run; a second identical call raises neither the arena's peak nor its reservation, so
    the first one gave back every block it took"""
    from fgdm_amd.engine import ContextCachePolicy
    i32 = C.c_int32
    levels = []
    for _ in range(2):
        x = x0.clone()
        p, keep = make(x, c, uc, n_log=2, log_steps=([0, 3], i32), x_inter_out=out.t.data_ptr())
        assert getattr(engine.lib, entry)(engine.h, C.byref(p), None) == 0
        torch.cuda.synchronize()
        levels.append(_levels(engine))
    out.check()
    assert torch.equal(out.t[1], x) and not torch.equal(x, x0)          # slot 1: x of the last step
    assert levels[0] == levels[1] and levels[0][0] > 0, levels
    engine._ctx_policy = ContextCachePolicy()                            # the raw calls registered their own context
    return x


def test_ancestral_argument_errors_come_before_any_launch(engine):
    x0, c, uc = _inputs()
    dev = torch.ones(S_ARG, *x0.shape, device='cuda')           # any valid device buffer of [S, B,4,H,W]
    out = guarded_out((2, *x0.shape), torch.float32)
    f = C.c_float
    coef = dict(sqrt_alphas_cumprod_t=([.5] * S_ARG, f), sqrt_one_minus_alphas_cumprod_t=([.5] * S_ARG, f))
    _runs_and_returns_its_workspace(engine, 'fgdm_sample_ancestral', _ancestral_params, x0, c, uc, out)      # warm: the arena holds its slabs
    out = guarded_out((2, *x0.shape), torch.float32)
    bad = _log_cases(out)
    bad.update({
        'struct_size too small': dict(struct_size=168),
        'struct_size too large': dict(struct_size=184),
        'reserved1 set': dict(reserved1=1),
        'mask without x0': dict(mask=dev.data_ptr(), q_noise=dev.data_ptr(), **coef),
        'mask without q_noise': dict(mask=dev.data_ptr(), x0=dev.data_ptr(), **coef),
        'mask without coefficients': dict(mask=dev.data_ptr(), x0=dev.data_ptr(), q_noise=dev.data_ptr()),
        'mask with one coefficient table': dict(mask=dev.data_ptr(), x0=dev.data_ptr(), q_noise=dev.data_ptr(),
                                                sqrt_alphas_cumprod_t=([.5] * S_ARG, f)),
        'a std without step_noise': dict(std=([0.0, 0.2, 0.0, 0.0], f)),
    })
    bad.update({f'{k} NULL': {k: None} for k in ('sqrt_recip_alphas_cumprod', 'sqrt_recipm1_alphas_cumprod', 'posterior_mean_coef1',
                                                 'posterior_mean_coef2', 'std')})
    _refused(engine, 'fgdm_sample_ancestral', _ancestral_params, bad, x0, c, uc, out)
    # with noise and a mask the same walk runs, and differs
    plain = _runs_and_returns_its_workspace(engine, 'fgdm_sample_ancestral', _ancestral_params, x0, c, uc, out)
    x = x0.clone()
    p, keep = _ancestral_params(x, c, uc, std=([0.3, 0.2, 0.1, 0.0], f), step_noise=dev.data_ptr(), mask=dev.data_ptr(),
                                x0=dev.data_ptr(), q_noise=dev.data_ptr(), **coef)
    assert engine.lib.fgdm_sample_ancestral(engine.h, C.byref(p), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(x, torch.ones_like(x))          # mask = 1 everywhere: q_sample(x0 = 1, noise = 1) with 0.5, 0.5
    assert not torch.equal(plain, x)
    from fgdm_amd.engine import ContextCachePolicy
    engine._ctx_policy = ContextCachePolicy()


def test_encode_argument_errors_come_before_any_launch(engine):
    x0, c, uc = _inputs()
    out = guarded_out((2, *x0.shape), torch.float32)
    _runs_and_returns_its_workspace(engine, 'fgdm_ddim_encode', _encode_params, x0, c, uc, out)
    out = guarded_out((2, *x0.shape), torch.float32)
    bad = _log_cases(out)
    bad.update({
        'struct_size too small': dict(struct_size=104),
        'struct_size too large': dict(struct_size=120),
        'cx NULL': dict(cx=None),
        'ce NULL': dict(ce=None),
    })
    _refused(engine, 'fgdm_ddim_encode', _encode_params, bad, x0, c, uc, out)
    _runs_and_returns_its_workspace(engine, 'fgdm_ddim_encode', _encode_params, x0, c, uc, out)


def test_workspace_is_back_at_its_level_after_the_python_routes(engine):
    """the walk (three segments, mask, logs) and the inversion (CFG, logs) through the Python layer, twice each"""
    from fgdm_amd import samplers
    x_T, c, uc = _inputs(3)
    kw, _ = _walk_kw('mask_intermediates', 3)

    def walk():
        m = _ldm(engine, True)
        m.max_loop_noise_bytes = 2 * 2 * x_T.numel() * 4
        torch.manual_seed(5)
        m.p_sample_loop(c, (3, 4, 8, 8), x_T=x_T, **kw)

    def encode():
        s = samplers.ControlDDIMSampler(_ldm(engine, False), device_loop=True)
        s.make_schedule(10, verbose=False)
        s.encode(x_T, c, 5, return_intermediates=2, unconditional_guidance_scale=3.0, unconditional_conditioning=uc)
    for call in (walk, encode):
        call()
        torch.cuda.synchronize()
        first = _levels(engine)
        call()
        torch.cuda.synchronize()
        assert _levels(engine) == first and first[0] > 0
