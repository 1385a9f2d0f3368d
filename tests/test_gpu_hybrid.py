"""Hybrid conditioning on the GPU: UNets fed cat([x] + c_concat, 1) (DiffusionWrapper 'hybrid', ldm/models/diffusion/ddpm.py:
1838-1841; SD-v1 inpainting, 9 input channels, and InstructPix2Pix, 8).  The pack kernel alone (fgdm_op_pack_xcat), the whole
network against the reference's goldens (tests/golden/hybrid*.npz) and the oracle, the bit identities of the cache and of the
CFG-pairs shortcut, the state errors, and a guided sampling through ControlDDIMSampler.  Whole-network gates: tests/common.py."""
import ctypes as C

import pytest
import torch

import golden_inputs as gi
import hybrid_inputs as hi
from common import CAP_CHAIN, CAP_EVAL, check_net, check_net_vs_oracle, gold, relerr
from fgdm_amd import _lib, models, samplers, synth
from guarded import guarded_in, guarded_out

pytestmark = pytest.mark.gpu

N, O, P = _lib.FLAG_NO_CONTROL, _lib.FLAG_USE_ORIGINAL, _lib.FLAG_CFG_PAIRS
SMALL9 = hi.cfg(9, gi.SMALL_CFG)
ERR_ARG, ERR_STATE = '(-1)', '(-3)'        # FGDM_ERR_ARG / FGDM_ERR_STATE as Engine._check words them


def build_engine(cfg):
    from fgdm_amd.engine import Engine
    e = Engine(cfg)
    for k, shape in e.param_shapes().items():
        e.load_tensor(k, synth.make_tensor(k, shape))
    e.finalize()
    return e


@pytest.fixture(scope='module')
def small9():
    e = build_engine(SMALL9)
    yield e
    e.close()


def _check(name, got, *a, **k):
    """check_net against goldens, check_net_vs_oracle against a callable; both print every error with its floor and gate
    (common.report), which is what profiles/hybrid_parity_errors.txt records"""
    return (check_net_vs_oracle if callable(a[0]) else check_net)(name, got, *a, **k)


# ---------------------------------------------------------------------------------------------------------------- 1. pack kernel
def _cin_pad(cin):
    return (cin + 7) // 8 * 8 if cin % 8 == 0 else (cin + 3) // 4 * 4


def _pack(x, c, B, Bc, H, W):
    """fgdm_op_pack_xcat on guarded buffers: x fp32 [B,4,H,W], c fp32 [Bc,Cc,H,W] (stored fp16 NHWC, as the engine keeps it)"""
    lib = _lib.load()
    Cc = c.shape[1]
    cp = _cin_pad(4 + Cc)
    xd = guarded_in(x.contiguous())
    cd = guarded_in(c.half().permute(0, 2, 3, 1).contiguous())
    out = guarded_out((B, H * W, cp), torch.float16)
    rc = lib.fgdm_op_pack_xcat(C.c_void_p(xd.data_ptr()), C.c_void_p(cd.data_ptr()), B, Bc, Cc, H, W, cp, C.c_void_p(out.data_ptr()), None)
    assert rc == 0
    torch.cuda.synchronize()
    return out.check().clone(), cp


@pytest.mark.parametrize('H,W', [(8, 8), (5, 7)])
@pytest.mark.parametrize('Cc', [1, 4, 5, 28])
def test_pack_kernel_is_bit_equal_to_cat_round_permute(Cc, H, W):
    assert _cin_pad(4 + Cc) == {1: 8, 4: 8, 5: 12, 28: 32}[Cc]
    for B, Bc in ((3, 3), (4, 2)):
        x = hi.x(B, H, W, seed=11 + Cc)
        c = hi._normal(f'hybrid.pack{Cc}', (Bc, Cc, H, W), seed=12)
        got, cp = _pack(x, c, B, Bc, H, W)
        full = c if Bc == B else torch.cat([c, c])                      # rows b and b + B/2 share row b
        want = torch.cat([x, full], 1).half().permute(0, 2, 3, 1).reshape(B, H * W, 4 + Cc).cuda()
        assert torch.equal(got[:, :, :4 + Cc].view(torch.int16), want.view(torch.int16))
        assert bool((got[:, :, 4 + Cc:].view(torch.int16) == 0).all())          # pad channels exactly +0
        if Bc != B:
            again, _ = _pack(x, full, B, B, H, W)                               # the half tensor repeated, Bc = B
            assert torch.equal(got.view(torch.int16), again.view(torch.int16))
            assert torch.equal(got[2:, :, 4:4 + Cc], got[:2, :, 4:4 + Cc])


@pytest.mark.parametrize('Cc', [4, 5])
def test_packed_rows_are_what_the_first_convolution_reads(Cc):
    """The pack kernel's output handed to fgdm_op_conv2d with C0 = 4 + Cc, which reads it with the row stride and the weight
    columns of the engine's own conv3_kmap: were _cin_pad above (or the header's rule) to drift from the engine's, the rows would
    be misread and this conv_in would be far off.  Reference: F.conv2d in float64 on the fp16-rounded input and weights, normwise
    1e-3 (the per-kernel bar of tests/test_gpu_narrow_ops.py; its measured worst case is 2.6e-4)."""
    lib = _lib.load()
    B, H, W, Cin, Cout = 2, 5, 7, 4 + Cc, 320
    x, c = hi.x(B, H, W, seed=41), hi._normal(f'hybrid.conv{Cc}', (B, Cc, H, W), seed=42)
    packed, cp = _pack(x, c, B, B, H, W)
    w = hi._normal(f'hybrid.convw{Cc}', (Cout, Cin, 3, 3), seed=43) * (9 * Cin) ** -0.5
    bias = hi._normal(f'hybrid.convb{Cc}', (Cout,), seed=44)
    xin, wd, bd = guarded_in(packed), w.cuda(), bias.cuda()
    out = guarded_out((B * H * W, Cout), torch.float16)
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = lib.fgdm_op_conv2d(p(xin), Cin, None, 0, p(wd), p(bd), None, None, B, H, W, Cout, 3, 1, 0, 0, 1.0, p(out.t), None)
    assert rc == 0
    torch.cuda.synchronize()
    got = out.check().view(B, H, W, Cout).permute(0, 3, 1, 2).cpu()
    ref = torch.nn.functional.conv2d(torch.cat([x, c], 1).half().double(), w.half().double(), bias.double(), padding=1)
    err = relerr(got, ref)
    print(f'pack -> conv_in, Cin {Cin} (cin_pad {cp}): rel_err={err:.3e} (tol 1.0e-03)')
    assert err < 1e-3


# ---------------------------------------------------------------------------------------------------------------- 2. whole network
def _oracle_fn(cfg, x, cc, t, ctx):
    from oracle import arch, nn as onn
    p = hi.params(arch.unet_param_shapes(cfg, adapter=False))
    return lambda: onn.unet_forward(p, cfg, torch.cat([x, cc], 1), t, ctx, prefix=hi.PREFIX)


@pytest.mark.parametrize('cin', hi.IN_CHANNELS)
def test_full_width_unet_vs_reference_goldens(cin):
    """LatentDiffusion(conditioning_key='hybrid').apply_model over the full-width UNet, 8x8, B = 2, t = (981, 1), against the
    reference's own apply_model (fp32 and under its autocast policy); and the bit identities of the 8x8 case that need no second
    engine: the [uc, c] batch with and without the pair flag, a sample alone, a second call served from the cache."""
    g, ga = gold('hybrid'), gold('hybrid_ac')
    m = models.LatentDiffusion(unet_config=hi.cfg(cin), conditioning_key='hybrid')
    try:
        e = m.engine
        assert e.config.in_channels == cin and e.config.use_adapter == 0
        assert not m.load_state_dict({k: synth.make_tensor(k, s) for k, s in e.param_shapes().items()})[0]
        x, t, ctx, cc = hi.x().cuda(), torch.tensor(hi.T).cuda(), hi.ctx().cuda(), hi.c_concat(cin - 4).cuda()
        cond = {'c_concat': [cc], 'c_crossattn': [ctx]}
        eps = m.apply_model(x, t, cond, use_original=True).clone()
        _check(f'hybrid UNet in_channels {cin}, 8x8', eps.cpu(), g[f'eps{cin}'], ga[f'eps{cin}'], cap=CAP_EVAL)
        assert torch.equal(m.apply_model(x, t, cond), eps) and e.concat_uploads == 1          # cache hit; no adapter either way
        assert torch.equal(m.apply_model(x[1:], t[1:], {'c_concat': [cc[1:].contiguous()], 'c_crossattn': [ctx[1:].contiguous()]}), eps[1:])
        # classifier-free-guidance batch [uc, c]: Bc = B/2 with the flag == Bc = B without it
        x2, t2, ctx2 = torch.cat([x, x]), torch.cat([t, t]), torch.cat([hi.ctx(seed=8).cuda(), ctx])
        e.set_concat(cc)
        paired = e.apply_model(x2, t2, ctx2, flags=N | P).clone()
        e.set_concat(torch.cat([cc, cc]))
        plain = e.apply_model(x2, t2, ctx2, flags=N).clone()
        assert torch.equal(paired, plain) and torch.equal(paired[2:], eps) and not torch.equal(paired[:2], eps)
        assert torch.equal(e.apply_model(x2, t2, ctx2, flags=N | P), paired)          # the flag with Bc = B: rows [0, B/2) are read
    finally:
        m.engine.close()


def test_non_square_latent_vs_oracle(small9):
    """16 x 24 latent at 9 channels, B = 1 and t = 501: conv_in's im2col rows and the pack kernel on a non-square grid.  On the
    REDUCED-DEPTH network (SMALL_CFG widths with 9 input channels), not the full-width one: what a non-square grid can break --
    the pack kernel, conv_in, the row arithmetic of the first levels -- is the same code there, and the CPU oracle's three modes
    of a full-width UNet at 384 pixels would take this test from under a second to the better part of a minute."""
    x, ctx, cc = hi.x(1, 16, 24, seed=31), hi.ctx(1, seed=32), hi.c_concat(5, 1, 16, 24, seed=33)
    t = torch.tensor([501])
    small9.set_concat(cc.cuda())
    got = small9.apply_model(x, t, ctx, flags=N)
    assert tuple(got.shape) == (1, 4, 16, 24)
    _check('hybrid UNet (reduced depth) in_channels 9, non-square 16x24, batch 1', got.cpu(), _oracle_fn(SMALL9, x, cc, t, ctx))


# ---------------------------------------------------------------------------------------------------------------- 3. bit identities
def test_cache_and_pairs_are_bit_identical(small9):
    e = small9
    x, t, ctx, cc = hi.x().cuda(), torch.tensor(hi.T).cuda(), hi.ctx().cuda(), hi.c_concat(5).cuda()
    m = models.LatentDiffusion(engine=e, conditioning_key='hybrid')
    cond = {'c_concat': [cc], 'c_crossattn': [ctx]}
    n0 = e.concat_uploads
    first = m.apply_model(x, t, cond).clone()
    assert torch.equal(m.apply_model(x, t, cond), first) and e.concat_uploads == n0 + 1        # second call: a cache hit
    # the [uc, c] batch: pair flag with the half tensor == no flag with the full one
    x2, t2, ctx2 = torch.cat([x, x]), torch.cat([t, t]), torch.cat([hi.ctx(seed=8).cuda(), ctx])
    paired = m.apply_model(x2, t2, {'c_concat': [cc], 'c_crossattn': [ctx2]}, cfg_pairs=True).clone()
    calls = e.pair_calls
    plain = m.apply_model(x2, t2, {'c_concat': [torch.cat([cc, cc])], 'c_crossattn': [ctx2]}).clone()
    assert e.pair_calls == calls and torch.equal(paired, plain) and torch.equal(paired[2:], first)
    assert not torch.equal(paired[:2], paired[2:])
    # the pair flag with the FULL tensor (equal halves, so the mirror keeps the flag): rows [0, B/2) of it serve the shared prefix
    full = m.apply_model(x2, t2, {'c_concat': [torch.cat([cc, cc])], 'c_crossattn': [ctx2]}, cfg_pairs=True)
    assert e.pair_calls == calls + 1 and torch.equal(full, paired)
    unequal = m.apply_model(x2, t2, {'c_concat': [torch.cat([torch.zeros_like(cc), cc])], 'c_crossattn': [ctx2]}, cfg_pairs=True)
    assert e.pair_calls == calls + 1 and torch.equal(unequal[2:], first) and not torch.equal(unequal[:2], paired[:2])
    # sample 1 of the batch of 2, evaluated alone
    alone = m.apply_model(x[1:], t[1:], {'c_concat': [cc[1:].contiguous()], 'c_crossattn': [ctx[1:].contiguous()]})
    assert torch.equal(alone, first[1:])
    # an in-place change is noticed, and gives what an engine that never saw the old tensor gives
    m.apply_model(x, t, cond)
    cc[:, 1:].mul_(0.5)
    changed = m.apply_model(x, t, cond).clone()
    assert not torch.equal(changed, first)
    fresh = build_engine(SMALL9)
    try:
        fresh.set_concat(cc.clone())
        assert torch.equal(fresh.apply_model(x, t, ctx, flags=N), changed)
    finally:
        fresh.close()


# ---------------------------------------------------------------------------------------------------------------- 4. state errors
def test_state_errors_launch_nothing_and_leave_engines_alone():
    x, t, ctx = hi.x().cuda(), torch.tensor(hi.T).cuda(), hi.ctx().cuda()
    e = build_engine(SMALL9)
    try:
        e.cache_context = False       # (the binding would project a new context through to_k / to_v ahead of the call)
        e.profile_begin(1)
        with pytest.raises(RuntimeError, match='no c_concat was registered') as err:
            e.apply_model(x, t, ctx, flags=N)
        assert ERR_STATE in str(err.value)
        assert sum(v['launches'] for v in e.profile_end().values()) == 0      # refused before the first launch
        e.cache_context = True
        for bad in (hi.c_concat(4), hi.c_concat(6)):                          # Cc must be in_channels - 4
            with pytest.raises(RuntimeError, match='in_channels - 4') as err:
                e.set_concat(bad.cuda())
            assert ERR_ARG in str(err.value)
        with pytest.raises(RuntimeError, match='no c_concat was registered'):      # a refused tensor registers nothing
            e.apply_model(x, t, ctx, flags=N)
        e.set_concat(hi.c_concat(5, H=8, W=16).cuda())
        with pytest.raises(RuntimeError, match='another latent size') as err:
            e.apply_model(x, t, ctx, flags=N)
        assert ERR_STATE in str(err.value)
        e.set_concat(hi.c_concat(5, H=16, W=8).cuda())
        with pytest.raises(RuntimeError, match='another latent size'):
            e.apply_model(x, t, ctx, flags=N)
        e.set_concat(hi.c_concat(5, B=3).cuda())
        with pytest.raises(RuntimeError, match='3 rows') as err:
            e.apply_model(x, t, ctx, flags=N)
        assert ERR_STATE in str(err.value)
        e.set_concat(None)                                                    # NULL clears the cache
        with pytest.raises(RuntimeError, match='no c_concat was registered'):
            e.apply_model(x, t, ctx, flags=N)
        with pytest.raises(RuntimeError, match='in_channels != 4'):
            e.apply_model_patches(x, t, ctx, (4, 4), (4, 4), torch.ones(4, 4), torch.ones(4))
        e.set_concat(hi.c_concat(5).cuda())
        assert bool(torch.isfinite(e.apply_model(x, t, ctx, flags=N)).all())  # the engine still works after all the refusals
        n = e.pair_calls
        with pytest.raises(RuntimeError, match='in_channels - 4'):            # a refused tensor also drops the one stored before it
            e.set_concat(hi.c_concat(6).cuda())
        with pytest.raises(RuntimeError, match='no c_concat was registered'):
            e.apply_model(torch.cat([x, x]), torch.cat([t, t]), torch.cat([ctx, ctx]), flags=N | P)
        assert e.pair_calls == n                                              # a refused call is not counted as a paired one
    finally:
        e.close()
    # a 4-channel engine refuses the call and computes what it computed before it
    e = build_engine(gi.SMALL_CFG)
    try:
        before = e.apply_model(x, t, ctx, flags=N).clone()
        with pytest.raises(RuntimeError, match='takes x alone') as err:
            e.set_concat(hi.c_concat(5).cuda())
        assert ERR_ARG in str(err.value)
        with pytest.raises(RuntimeError, match='takes x alone'):
            e.set_concat(None)
        assert torch.equal(e.apply_model(x, t, ctx, flags=N), before)
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------------------- 5. sampling
@pytest.mark.parametrize('uncond_image', ['same', 'clone', 'zeros'])
def test_guided_sampling_vs_oracle(uncond_image):
    """ControlDDIMSampler over a hybrid LatentDiffusion, S = 3, scale 7.5, B = 2, 8x8: cond and uncond with the same c_concat run
    as one paired batch (the same tensor object: the half-batch tensor; an equal CLONE: the concatenated tensor, whose halves the
    mirror finds equal), an uncond with a zero image as one unpaired batch with c_concat concatenated -- both against the same
    three steps driven through the oracle (two sequential calls per step).  The model and the oracle carry a 999-step schedule:
    S = 3 does not divide the usual 1000 -- make_ddim_timesteps then returns FOUR timesteps, the last one 1000, and the
    reference's make_schedule (like this repo's) indexes alphas_cumprod out of range (util.py:46-60); range(0, 999, 333) + 1 is the
    three timesteps 1, 334, 667."""
    from oracle import arch, nn as onn, samplers as osamp, schedule
    model = models.LatentDiffusion(unet_config=SMALL9, conditioning_key='hybrid', timesteps=999)
    try:
        e = model.engine
        assert not model.load_state_dict({k: synth.make_tensor(k, s) for k, s in e.param_shapes().items()})[0]
        B, S = 2, 3
        x_T, c, uc, cc = hi.x(seed=21), hi.ctx(seed=22), hi.ctx(seed=23), hi.c_concat(5, seed=24)
        ucc = torch.zeros_like(cc) if uncond_image == 'zeros' else cc
        cc_d = cc.cuda()
        cond = {'c_concat': [cc_d], 'c_crossattn': [c.cuda()]}
        ucond = {'c_concat': [{'same': cc_d, 'clone': cc_d.clone(), 'zeros': ucc.cuda()}[uncond_image]], 'c_crossattn': [uc.cuda()]}
        out, _ = samplers.ControlDDIMSampler(model).sample(S, B, (4, 8, 8), cond, verbose=False, eta=0.0, x_T=x_T.cuda(),
                                                           unconditional_guidance_scale=7.5, unconditional_conditioning=ucond)
        # one 2B batch per step either way; the pair flag only where the halves share the image; one upload for the whole sampling
        assert e.pair_calls == (0 if uncond_image == 'zeros' else S) and e.concat_uploads == 1
        p = hi.params(arch.unet_param_shapes(SMALL9, adapter=False))
        fn = lambda x, t, cd: onn.unet_forward(p, SMALL9, torch.cat([x, cd[0]], 1), t, cd[1], prefix=hi.PREFIX)
        run = lambda: osamp.ddim_sample(fn, schedule.register_schedule(timesteps=999), S, x_T.shape, (cc, c), x_T, scale=7.5, uc=(ucc, uc),
                                        cfg_mode='sequential')[0]
        _check(f'hybrid LatentDiffusion + ControlDDIMSampler, 3 steps CFG 7.5, uncond image: {uncond_image}', out.cpu(), run,
               cap=CAP_CHAIN)
    finally:
        model.engine.close()
