"""SD-2.1-base style networks on the GPU: the d = 64 instantiations of every attention kernel family under the engine's own call,
one SpatialTransformer with nn.Linear projections, the SD21_SMALL UNet and UNet + ControlNet against the reference's goldens
(tests/golden/sd21_*.npz, tools/make_goldens_sd21.py), and one sampler pass.

Attention bars are those tests/test_gpu_attention_calls.py applies to d = 40 / 80: normwise TOL and blockwise 2 TOL on unit
operands, regime_bars() in the logit regimes.  Network bars are tests/common.py::check_net's, per block the flat 1e-3."""
import ctypes as C
import math

import pytest
import torch

import attention_dispatch as AD
import attention_dispatch_d64 as AD64
import sd21_inputs as si
from common import check_net, gold, net_tol, relerr, report
from guarded import guarded_in, guarded_out, tile_err
from fgdm_amd import synth
from test_gpu_attention_calls import (LOG2E, NAN16, REGIMES, check_regime_shape, emulate, make_vt, prescale, reference, regime_bars,
                                      regime_inputs, unit_inputs)
from test_gpu_ops import TOL, _st, close

pytestmark = pytest.mark.gpu

B, H, D = 2, 5, 64          # an odd head count: the block -> (batch, head) mapping cannot hide behind a power of two
CC = H * D
PAD_COLS, PAD_ROWS = 8, 3   # output columns beyond H d in every row, and whole rows beyond B T: poisoned, must stay untouched


@pytest.fixture(scope='module')
def lib():
    from fgdm_amd import _lib
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return _lib.load()


def _case(T, Tk, kernel):
    return (kernel, B, H, T, Tk, D, True)          # the case tuple of test_gpu_attention_calls


def _id(c):
    return f'{AD.KERNEL_NAMES[c[2]]}_T{c[0]}Tk{c[1]}'


def launch_engine_layout(lib, q, k, v, T, Tk, kernel):
    """One call as Engine::attn_fwd makes it: self-attention (T == Tk) reads Q | K as the column halves of ONE [B T, 2 C] buffer,
    cross-attention reads compact Q and K; V^T is wider than its keys (ldvt > roundup(Tk, 64), NaN beyond); Q is pre-scaled.
    The output has PAD_COLS poisoned columns per row and PAD_ROWS poisoned rows behind it."""
    q2, k2 = q.reshape(B * T, CC).half(), k.reshape(B * Tk, CC).half()
    if T == Tk:
        qk = guarded_in(torch.cat([q2, k2], 1).contiguous())
        qp, kp, ldq, ldk, keep = qk.data_ptr(), qk.data_ptr() + 2 * CC, 2 * CC, 2 * CC, [qk]
    else:
        qb, kb = guarded_in(q2.contiguous()), guarded_in(k2.contiguous())
        qp, kp, ldq, ldk, keep = qb.data_ptr(), kb.data_ptr(), CC, CC, [qb, kb]
    ldvt = (Tk + 63) // 64 * 64 + 64
    vtd = guarded_in(make_vt(v, B, Tk, CC, ldvt, NAN16).contiguous())
    ldo = CC + PAD_COLS
    out = guarded_out((B * T + PAD_ROWS, ldo), torch.half)
    rc = lib.fgdm_op_attention_ex(C.c_void_p(qp), ldq, C.c_void_p(kp), ldk, C.c_void_p(vtd.data_ptr()), ldvt,
                                  C.c_void_p(out.data_ptr()), ldo, B, H, T, Tk, D, 1, _st())
    assert rc == 0, rc
    torch.cuda.synchronize()
    got = lib.fgdm_debug_last_attention_kernel()
    assert got == kernel == AD64.expected_kernel_d64(T, Tk), f'ran on {AD.KERNEL_NAMES.get(got)}, written for {AD.KERNEL_NAMES[kernel]}'
    region = (slice(0, B * T), slice(0, CC))
    out.check(region)
    out.assert_untouched((slice(0, B * T), slice(CC, ldo)))
    out.assert_untouched((slice(B * T, B * T + PAD_ROWS), slice(None)))
    keep.append(vtd)
    return out.t[region], keep


@pytest.mark.parametrize('shape', AD64.D64_CASES, ids=_id)
def test_attention_d64_engine_call(lib, shape):
    T, Tk, kernel = shape
    case = _case(T, Tk, kernel)
    q, k, v = unit_inputs(case, seeds=(241, 242, 243))          # unit randn, key 70 spiked against query 0 of head 0
    qs = prescale(q, D)
    ref, _ = reference(qs, k, v, B, H, D, 1.0)
    got, keep = launch_engine_layout(lib, qs, k, v, T, Tk, kernel)
    what = f'attention d64 engine call {_id(shape)}'
    assert relerr(got.float().cpu(), ref) < TOL, what
    close(what, got, ref, local=2 * TOL)


@pytest.mark.parametrize('name', REGIMES)
@pytest.mark.parametrize('shape', AD64.D64_CASES, ids=_id)
def test_attention_d64_logit_regimes(lib, shape, name):
    T, Tk, kernel = shape
    case = _case(T, Tk, kernel)
    q, k, v = regime_inputs(name, case)
    q = prescale(q, D)
    ref, s = reference(q, k, v, B, H, D, 1.0)
    check_regime_shape(name, case, s)
    emu = emulate(q, k, v, B, H, D, True)
    bar, bar_blk = regime_bars(name, case, relerr(emu, ref), tile_err(emu, ref))
    got, keep = launch_engine_layout(lib, q, k, v, T, Tk, kernel)
    err, blk = relerr(got.float().cpu(), ref), tile_err(got, ref)
    print(f'{AD.KERNEL_NAMES[kernel]} d64 T{T} Tk{Tk} {name}: rel_err={err:.3e} tile_err={blk:.3e} bars {bar:.1e} / {bar_blk:.1e}')
    assert err < bar, (_id(shape), name, err, bar)
    assert blk < bar_blk, (_id(shape), name, 'tile_err', blk, bar_blk)


# ------------------------------------------------------------------------------------------------------------------ networks
@pytest.fixture(scope='module')
def sd21_engine():
    from test_gpu_nets import build_engine
    e = build_engine(si.SD21_SMALL, si.rename, n_controlnets=1)
    yield e
    e.close()


def test_spatial_transformer_linear_projections(sd21_engine):
    """input_blocks.1.1 of SD21_SMALL IS SpatialTransformer(320, 5 heads of 64, context 1024, use_linear): loaded with the weights
    the fixture's module had, run alone.  Per-block bar: 1e-3 against the reference's fp32 output."""
    from fgdm_amd.engine import Engine
    pre = 'model.diffusion_model.input_blocks.1.1.'
    e = Engine(si.SD21_SMALL)
    try:
        for k, shape in e.param_shapes().items():
            e.load_tensor(k, synth.make_tensor('sd21_st.' + k[len(pre):] if k.startswith(pre) else k, shape))
        e.finalize()
        got = e.run_block(pre, si.get('st_x'), ctx=si.get('ctx'))
    finally:
        e.close()
    y = torch.from_numpy(gold('sd21_st')['y'])
    err = report('block SpatialTransformer C320 T256 d64 linear vs reference fp32', relerr(got.cpu().view_as(y), y), 1e-3)
    assert err <= 1e-3


def test_sd21_unet_and_controlnet_vs_reference_goldens(sd21_engine):
    from fgdm_amd import _lib
    g, ga = gold('sd21_nets'), gold('sd21_nets_ac')
    x, ctx, t = si.get('x'), si.get('ctx'), torch.from_numpy(g['t'])
    e = sd21_engine.apply_model(x, t, ctx, flags=_lib.FLAG_NO_CONTROL)
    check_net('SD21_SMALL UNet 16x16', e.cpu(), g['eps'], ga['eps'])
    sd21_engine.set_hint(0, si.hint().cuda())
    e = sd21_engine.apply_model(x, t, ctx, control_scales=si.CTRL_SCALES)
    check_net('SD21_SMALL UNet+ControlNet 16x16', e.cpu(), g['eps_ctrl'], ga['eps_ctrl'])
    # ... and as the 2B batch of a classifier-free-guidance step: rows b and b + B differ only in the context
    x2, t2 = torch.cat([x, x]), torch.cat([t, t])
    ctx2 = torch.cat([torch.from_numpy(synth._rng('sd21.uc', 7).standard_normal(tuple(ctx.shape), dtype='float32')), ctx])
    pair = sd21_engine.apply_model(x2, t2, ctx2, control_scales=si.CTRL_SCALES, flags=_lib.FLAG_CFG_PAIRS).cpu()
    assert torch.equal(pair[2:], e.cpu())
    check_net('SD21_SMALL UNet+ControlNet 16x16, CFG pair', pair[2:], g['eps_ctrl'], ga['eps_ctrl'])
    plain = sd21_engine.apply_model(x2, t2, ctx2, control_scales=si.CTRL_SCALES).cpu()
    assert torch.equal(pair, plain)


def test_sd21_batch_rows_are_independent(sd21_engine):
    from fgdm_amd import _lib
    x, ctx, t = si.get('x'), si.get('ctx'), torch.tensor(si.T_PAIR)
    f = _lib.FLAG_NO_CONTROL
    full = sd21_engine.apply_model(x, t, ctx, flags=f).cpu()
    assert torch.equal(full, sd21_engine.apply_model(x, t, ctx, flags=f).cpu())
    for b in range(2):
        one = sd21_engine.apply_model(x[b:b + 1], t[b:b + 1], ctx[b:b + 1], flags=f).cpu()
        assert torch.equal(full[b:b + 1], one), b


def test_sd21_control_ddim_sampler_vs_host_loop():
    """4 DDIM steps (3 do not divide the 1000 training steps: make_ddim_timesteps, here as in the reference, then selects timestep
    1000, which the schedule does not have) with CFG through ControlDDIMSampler on a ControlLDM built from the SD-2 config, against a host-side loop over
    apply_model with the sampler's own tables.  Both sides run the same engine, so what separates them is the sampler arithmetic
    (fused fp32 kernel against torch fp32) fed back through four evaluations: held to net_tol(0) = 1e-3, the network bound where
    no autocast floor widens it."""
    from fgdm_amd import models, samplers
    model = models.ControlLDM(unet_config=si.SD21_SMALL, control_stage_config=dict(si.SD21_SMALL, hint_channels=3))
    try:
        sd = {k: synth.make_tensor(si.rename(k), s) for k, s in model.engine.param_shapes().items()}
        missing, _ = model.load_state_dict(sd)
        assert not missing
        model.control_scales = list(si.CTRL_SCALES)
        x_T, c, hint = si.get('x').cuda(), si.get('ctx').cuda(), si.hint().cuda()
        uc = torch.from_numpy(synth._rng('sd21.uc', 7).standard_normal(tuple(c.shape), dtype='float32')).cuda()
        cond, ucond = {'c_concat': [hint], 'c_crossattn': [c]}, {'c_concat': [hint], 'c_crossattn': [uc]}
        scale = 7.5
        smp = samplers.ControlDDIMSampler(model)
        out, _ = smp.sample(4, 2, (4, 16, 16), cond, verbose=False, eta=0.0, x_T=x_T.clone(), unconditional_guidance_scale=scale,
                            unconditional_conditioning=ucond)
        assert bool(torch.isfinite(out).all()) and len(smp.ddim_timesteps) == 4
        x = x_T.clone()
        steps = [int(v) for v in smp.ddim_timesteps]
        for i in reversed(range(len(steps))):
            t = torch.full((2,), steps[i], dtype=torch.long, device=x.device)
            e_c, e_u = model.apply_model(x, t, cond), model.apply_model(x, t, ucond)
            e = e_u + scale * (e_c - e_u)
            a, ap = float(smp.ddim_alphas[i]), float(smp.ddim_alphas_prev[i])
            x0 = (x - math.sqrt(1 - a) * e) / math.sqrt(a)
            x = math.sqrt(ap) * x0 + math.sqrt(1 - ap) * e
        err = report('SD21_SMALL ControlDDIMSampler 4 steps CFG 7.5 vs host loop over apply_model', relerr(out.cpu(), x.cpu()), net_tol(0.0))
        assert err < net_tol(0.0)
    finally:
        model.engine.close()
