"""The DPM-Solver program loop on the GPU (fgdm_sample_dpm_solver / k_dpm_program_step, fgdm_amd/dpm_solver.py).

  * the step kernel alone (fgdm_op_dpm_program_step) against a host emulation with the kernel's explicit roundings
    (tests/dpm_solver_cases.py: emulate_step), bit for bit, on poisoned, guarded buffers;
  * whole samplings: the device loop against the per-step route on the same engine from the same x_T, bit for bit;
  * the default configuration (multistep order 2, time_uniform, data prediction) against DPMSolverSampler: the two round the
    second-order update differently (one fma chain here, two axpby there), so they agree to fp32 rounding, not to the bit;
  * malformed programs are refused before anything is launched."""
import ctypes as C

import numpy as np
import pytest
import torch

import dpm_solver_cases as cases
import golden_inputs as gi
import test_gpu_multistep_loop as base
from common import relerr
from fgdm_amd import synth
from guarded import guarded_in, guarded_out

pytestmark = pytest.mark.gpu

ERR_ARG = -1
BASE, H0, H1, H2, M = 0, 1, 2, 3, 4


@pytest.fixture(scope='module')
def engine():
    e = base._build(gi.SMALL_CFG, n_controlnets=1)
    yield e
    e.close()


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


# ------------------------------------------------------------------------------------------------------------ the kernel alone
CFG, CONV_X, CONV_E = 7.5, 1.3971, -0.9757
COEFS = [0.8312, 0.2714, -0.0931, 0.0417, -0.6113]            # none of them a power of two
ORDERS = ([BASE, M, H0, H1, H2], [M, H2, BASE, H0, H1], [H1, H1, M, BASE, M])


def _launch(lib, d, n, planes, coefs, cfg_on, data, slot, null=(), alias=()):
    """one launch on fresh copies of the inputs `d`; returns (outputs by name, the three history planes after the launch).
    alias: 'x_out' (the base plane itself), 'xin_a' (x_eval itself)"""
    x_eval, bs = guarded_in(d['x_eval']), guarded_in(d['base'])
    hist = [guarded_out((n,), torch.float32) for _ in range(3)]
    for h, k in zip(hist, ('h0', 'h1', 'h2')):
        h.t.copy_(d[k])
    outs = {k: None if k in null or k in alias else guarded_out((n,), torch.float32) for k in ('x_out', 'xin_a', 'xin_b')}
    aliased = {'x_out': bs, 'xin_a': x_eval}
    ptr = lambda k: _p(aliased[k]) if k in alias else _p(outs[k] and outs[k].t)
    nt = len(planes)
    rc = lib.fgdm_op_dpm_program_step(_p(x_eval), _p(d['ec']), _p(d['eu'] if cfg_on else None), CFG, CONV_X if data else 0.0, CONV_E,
                                      _p(bs), *[_p(h.t) for h in hist], slot, nt, (C.c_int32 * nt)(*planes), (C.c_float * nt)(*coefs),
                                      ptr('x_out'), ptr('xin_a'), ptr('xin_b'), n, None)
    torch.cuda.synchronize()
    assert rc == 0
    got = {k: g.check() for k, g in outs.items() if g is not None}
    if 'x_out' in alias:
        got['x_out'] = bs
    else:
        assert torch.equal(bs, d['base'])
    if 'xin_a' in alias:
        got['xin_a'] = x_eval
    else:
        assert torch.equal(x_eval, d['x_eval'])
    for h in hist:
        h.check_guards()
    return got, [h.t for h in hist]


@pytest.mark.parametrize('n', [1, 255, 257, 4099])
def test_step_kernel_equals_the_host_emulation(n):
    from fgdm_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(n)
    host = {k: torch.randn(n, generator=g) for k in ('x_eval', 'base', 'h0', 'h1', 'h2', 'ec', 'eu')}
    d = {k: (guarded_in(v) if k in ('ec', 'eu') else v.cuda()) for k, v in host.items()}
    a = {k: v.numpy() for k, v in host.items()}

    def want(planes, coefs, cfg_on, data):
        return cases.emulate_step(a['x_eval'], a['ec'], a['eu'] if cfg_on else None, CFG, CONV_X if data else 0.0, CONV_E, a['base'],
                                  [a['h0'], a['h1'], a['h2']], planes, coefs)

    def check(planes, coefs, cfg_on, data, slot, **kw):
        got, hist = _launch(lib, d, n, planes, coefs, cfg_on, data, slot, **kw)
        m, acc = want(planes, coefs, cfg_on, data)
        for k, v in got.items():
            assert np.array_equal(v.cpu().numpy().view(np.int32), acc.view(np.int32)), (k, planes, cfg_on, data, slot, kw)
        for s, (h, k) in enumerate(zip(hist, ('h0', 'h1', 'h2'))):      # the slot's plane holds m, the others are untouched
            ref = m if s == slot else a[k]
            assert np.array_equal(h.cpu().numpy().view(np.int32), ref.view(np.int32)), ('hist', s, planes, slot)
        return got

    for order in ORDERS:
        for nt in range(1, 6):
            for cfg_on in (True, False):
                for data in (True, False):
                    got = check(order[:nt], COEFS[:nt], cfg_on, data, slot=nt % 3)      # (slot nt % 3 is read by some of them)
                    assert set(got) == {'x_out', 'xin_a', 'xin_b'}
    full = ORDERS[0]
    check(full, COEFS, True, True, slot=-1)                                             # nothing stored
    for slot in (0, 1, 2):                                                               # the slot's plane is one this record reads
        check(full, COEFS, True, True, slot=slot)
    check(full, COEFS, True, True, slot=0, alias=('x_out',))                            # x_out is the base plane
    check(full, COEFS, True, True, slot=1, alias=('xin_a',))                            # xin_a is x_eval, as in the device loop
    check(full, COEFS, False, False, slot=2, alias=('x_out', 'xin_a'))
    for k in ('x_out', 'xin_a', 'xin_b'):                                               # every optional output NULL in turn
        assert k not in check(full, COEFS, True, True, slot=0, null=(k,))
    assert check([M], [1.0], True, True, slot=-1, null=('xin_a', 'xin_b'))              # denoise_to_zero's record: x = m


# ------------------------------------------------------------------------------------------------------------ whole samplings
def _solver(model, c, uc, scale, px0, loop):
    from fgdm_amd import dpm_solver as ds
    ns = ds.NoiseScheduleVP('discrete', alphas_cumprod=model.alphas_cumprod)
    fn = ds.model_wrapper(model, ns, guidance_type='classifier-free', condition=c, unconditional_condition=uc, guidance_scale=scale)
    return ds.DPM_Solver(fn, ns, predict_x0=px0, device_loop=loop)


def _guard(e, monkeypatch):
    real, runs = e.sample_dpm_solver, []

    def run(x_T, *a, **k):
        gx = guarded_out(tuple(x_T.shape), torch.float32)
        out = real(x_T, *a, **k, out=gx.t)
        torch.cuda.synchronize()
        gx.check()
        runs.append(len(a[3]['t_float']))
        return out
    monkeypatch.setattr(e, 'sample_dpm_solver', run)
    return runs


LOOP_CASES = {
    'multistep_o3_S5_cfg_B2': (2, 7.5, True, dict(steps=5, order=3, method='multistep')),
    'singlestep_o3_S6_B1': (1, 1.0, False, dict(steps=6, order=3, method='singlestep')),
    'multistep_o2_S4_eps_cfg': (2, 7.5, False, dict(steps=4, order=2, method='multistep')),
    'singlestep_o3_S7_taylor_dz_cfg': (2, 5.0, True, dict(steps=7, order=3, method='singlestep', solver_type='taylor', denoise_to_zero=True,
                                                          skip_type='logSNR')),
}


@pytest.mark.parametrize('name', list(LOOP_CASES))
def test_device_loop_equals_per_step_route(engine, monkeypatch, name):
    B, scale, px0, kw = LOOP_CASES[name]
    runs = _guard(engine, monkeypatch)
    x_T, c, uc = base._inputs(B, 8, 8)
    m = base._ldm(engine)
    per_step = _solver(m, c, uc, scale, px0, False).sample(x_T, **kw)
    assert not runs
    loop = _solver(m, c, uc, scale, px0, True).sample(x_T, **kw)
    assert runs == [kw['steps'] + int(kw.get('denoise_to_zero', False))], 'the device loop did not take this sampling over'
    assert torch.equal(per_step, loop) and bool(torch.isfinite(loop).all()) and not torch.equal(loop, x_T)


def test_control_ldm_with_a_hint(engine, monkeypatch):
    runs = _guard(engine, monkeypatch)
    x_T, c, _ = base._inputs()
    hint = torch.from_numpy(synth.hint(2, res=64, seed=903)).cuda()
    m = base._cldm(engine)
    kw = dict(steps=3, order=2, method='multistep')
    cond = lambda h: {'c_concat': [h], 'c_crossattn': [c]}
    per_step = _solver(m, cond(hint), None, 1.0, True, False).sample(x_T, **kw)
    loop = _solver(m, cond(hint), None, 1.0, True, True).sample(x_T, **kw)
    assert runs == [3] and torch.equal(per_step, loop)
    moved = _solver(m, cond(hint.flip(-1).contiguous()), None, 1.0, True, True).sample(x_T, **kw)      # ... and the hint matters
    assert not torch.equal(moved, loop)


# relerr of the new route to DPMSolverSampler measured on an MI355X, per-step route and device loop alike
# (profiles/dpm_solver_parity_errors.txt)
DEFAULT_PARITY_MEASURED = 5.191e-8


def test_default_configuration_agrees_with_dpmsolversampler(engine):
    """multistep order 2, time_uniform, data prediction, S = 4: same coefficients (to fp32 equality, tests/test_dpm_solver_host.py),
    same network, and the first-order updates round alike (fma(c1, x, round(cm0 m0))); the second-order update fuses cm1 m1 into
    the sum here, where axpby(axpby(.), 1, m1, cm1) there rounds that product first.  Bound: 4x the distance measured on an MI355X
    (5.191e-8), and never looser than 1e-5 relative.  (With x leading the chain instead, so that every update rounded differently,
    the distance was 7.0e-4: the fp16 network amplifies a one-ulp change of every element of x_T to 7.4e-4 over these 4 steps.)"""
    from fgdm_amd import samplers
    x_T, c, uc = base._inputs()
    m = base._ldm(engine)
    old, _ = samplers.DPMSolverSampler(m).sample(4, 2, (4, 8, 8), c, verbose=False, x_T=x_T, unconditional_guidance_scale=7.5,
                                                 unconditional_conditioning=uc)
    for loop in (False, True):
        new = _solver(m, c, uc, 7.5, True, loop).sample(x_T, steps=4, order=2, method='multistep')
        err = relerr(new, old)
        print(f'default configuration, device_loop={loop}: relerr to DPMSolverSampler {err:.3e}')
        bound = min(1e-5, 4 * DEFAULT_PARITY_MEASURED)
        assert err <= bound, (loop, err, bound)


# ------------------------------------------------------------------------------------------------------------ malformed programs
def _params(x_, c_, uc_, **over):
    from fgdm_amd import _lib, dpm_solver as ds
    from oracle import schedule
    prog = ds.dpm_solver_program(ds.NoiseScheduleVP('discrete', alphas_cumprod=schedule.register_schedule()['alphas_cumprod']), 4, 2,
                                 'time_uniform', 'multistep', True)
    keep = []
    p = _lib.FgdmDpmSolverParams()
    p.struct_size = C.sizeof(p)
    p.x, p.cond, p.uncond = x_.data_ptr(), c_.data_ptr(), uc_.data_ptr()
    for k in ('t_float', 'conv_x', 'conv_e'):
        setattr(p, k, base._arr(keep, prog[k]))
    for k in ('slot', 'nterms', 'dest'):
        setattr(p, k, base._arr(keep, prog[k], C.c_int32))
    p.plane = base._arr(keep, [v for r in prog['plane'] for v in r], C.c_int32)
    p.coef = base._arr(keep, [v for r in prog['coef'] for v in r])
    p.cfg_scale, p.n_eval, p.B, p.H, p.W, p.flags = 7.5, 4, x_.shape[0], x_.shape[2], x_.shape[3], _lib.FLAG_NO_CONTROL
    for k, v in over.items():
        setattr(p, k, base._arr(keep, *v) if isinstance(v, tuple) else v)
    return p, keep, prog


def test_malformed_programs_are_refused_before_any_launch(engine):
    from fgdm_amd.engine import ContextCachePolicy
    x0, c, uc = base._inputs()
    i32 = C.c_int32
    _, _, prog = _params(x0, c, uc)
    planes = [v for r in prog['plane'] for v in r]
    unwritten = list(planes)
    unwritten[5 + 2] = H0 + 2                    # record 1 reads history slot 2: records 0 and 1 wrote 0 and (now) 1 only
    bad = {
        'a read of an unwritten slot': (dict(plane=(unwritten, i32)), b'record 1: reads history slot 2'),
        'nterms = 6': (dict(nterms=([2, 6, 3, 2], i32)), b'record 1: nterms 6'),
        'nterms = 0': (dict(nterms=([0, 3, 3, 2], i32)), b'record 0: nterms 0'),
        'slot 3': (dict(slot=([0, 3, -1, -1], i32)), b'record 1: slot 3'),
        'plane 5': (dict(plane=([4, 5] + planes[2:], i32)), b'record 0: unknown plane 5'),
        'destination 0': (dict(dest=([1, 1, 0, 1], i32)), b'record 2: unknown destination'),
        'last record to the evaluation input': (dict(dest=([1, 1, 1, 2], i32)), b'last record'),
        'struct_size too small': (dict(struct_size=128), b'struct_size'),
        'struct_size too large': (dict(struct_size=144), b'struct_size'),
        'reserved1 set': (dict(reserved1=1), b'reserved'),
        'no records': (dict(n_eval=0), b'n_eval'),
        'coef NULL': (dict(coef=None), b'NULL'),
    }
    for why, (over, msg) in bad.items():
        x = guarded_out(tuple(x0.shape), torch.float32)
        x.t.copy_(x0)
        p, keep, _ = _params(x.t, c, uc, **over)
        rc = engine.lib.fgdm_sample_dpm_solver(engine.h, C.byref(p), None)
        torch.cuda.synchronize()
        assert rc == ERR_ARG, why
        assert torch.equal(x.t, x0), why                       # nothing was launched: the state is untouched
        x.check_guards()
        err = engine.lib.fgdm_last_error(engine.h)
        assert b'fgdm_sample_dpm_solver' in err and msg in err, (why, err)
    x = x0.clone()
    p, keep, _ = _params(x, c, uc)                            # the same parameters without a defect run
    assert engine.lib.fgdm_sample_dpm_solver(engine.h, C.byref(p), None) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(x).all()) and not torch.equal(x, x0)
    engine._ctx_policy = ContextCachePolicy()
