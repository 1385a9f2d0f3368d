"""Text contexts longer than one 77-token CLIP chunk on the GPU (cat(c_crossattn, 1), ddpm.py:1835-1837 / cldm.py:836-849; the
three-chunk [B, 231, 768] context of controlnet/cldm/hack.py:23-68).

  * fgdm_op_attention over 96 < Tk <= 256 (the key-resident long text-attention kernel where it is dispatched, the general kernels
    elsewhere and under FGDM_ATTN_CROSS_LONG=0): guarded, poisoned buffers and the blockwise bound of tests/test_gpu_ops.py, same
    TOL as test_attention;
  * apply_model of the full-width UNet / ControlLDM against goldens from the reference's own modules (tests/golden/long_context*.npz)
    under check_net's existing rule;
  * bit-for-bit equivalences of the engine's paths (part list vs joined tensor, cached vs passed context, CFG-pair prefix sharing,
    device loop vs Python loop, token-count switches) and the sampler's two-call route for unequal token counts;
  * clip_skip and the chunked encoding."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

import golden_inputs as gi
import long_context_inputs as li
from attention_dispatch import expected_kernel
from common import check_net, gold, net_tol, params, relerr, report
from fgdm_amd import synth
from guarded import guarded_in, guarded_out
from test_gpu_ops import TOL, close, din, h16, rnd, _p, _st

pytestmark = pytest.mark.gpu

ATT_TK = (97, 128, 129, 154, 160, 161, 231, 255, 256)
ATT_D = (40, 80, 160)
# (T, B): ragged T (a wave's last chunk partly / wholly past the end), one and several chunks per wave, B up to 3
ATT_TB = ((128, 3), (700, 2), (1024, 1), (4096, 1))
HEADS = 4


@pytest.fixture(scope='module')
def lib():
    from fgdm_amd import _lib
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return _lib.load()


def spike_keys(Tk):
    """one key in the first, a middle and the last 32-key sub-tile"""
    ns = (Tk + 31) // 32
    return (5, (ns // 2) * 32 + 7, Tk - 1)


@pytest.mark.parametrize('d', ATT_D)
@pytest.mark.parametrize('Tk', ATT_TK)
def test_attention_long_text_contexts(lib, Tk, d):
    Hh, Cc = HEADS, HEADS * d
    Tkp = (Tk + 63) // 64 * 64
    split = lambda t, B: t.view(B, -1, Hh, d).permute(0, 2, 1, 3)
    for T, B in ATT_TB:
        if T == 4096 and d != 40:
            continue
        q0, k0, v = h16(rnd((B, T, Cc), 141)), h16(rnd((B, Tk, Cc), 142)), h16(rnd((B, Tk, Cc), 143))
        vt = torch.zeros(B, Cc, Tkp, dtype=torch.half)      # pad columns Tk <= t < Tkp zero: the engine's contract for V^T
        vt[:, :, :Tk] = v.permute(0, 2, 1).half()
        qd, vtd = din(q0.half()), din(vt)
        for key in spike_keys(Tk):
            k = k0.clone()
            k[:, key, :d] = q0[:, 0, :d] * 4.0              # the row maximum of query 0 / head 0 sits in that sub-tile
            sim = torch.matmul(split(q0, B), split(k, B).transpose(-1, -2)) * d ** -0.5
            assert int(sim[0, 0, 0].argmax()) == key
            ref = torch.matmul(sim.softmax(-1), split(v, B)).permute(0, 2, 1, 3).reshape(B, T, Cc)
            out = guarded_out((B, T, Cc), torch.half)
            kd = din(k.half())                               # K rows past Tk (of the last sample) sit in NaN guards
            rc = lib.fgdm_op_attention(_p(qd), Cc, _p(kd), Cc, _p(vtd), Tkp, _p(out.t), Cc, B, Hh, T, Tk, d, _st())
            assert rc == 0
            assert lib.fgdm_debug_last_attention_kernel() == expected_kernel(T, Tk, d), (T, Tk, d)
            torch.cuda.synchronize()
            what = f'attention long context B{B} H{Hh} T{T} Tk{Tk} d{d} spike@{key}'
            e = relerr(out.check().float().cpu(), ref)
            print(f'{what}: {e:.3e}')
            assert e < TOL, what
            close(what, out.t.reshape(B * T, Cc), ref.reshape(B * T, Cc), local=2 * TOL)


def test_attention_long_text_contexts_on_the_general_kernels():
    """FGDM_ATTN_CROSS_LONG=0 sends Tk > 96 back to the dispatch of before (same-box A/B runs), so that path stays under the same
    cases.  The knob is read once per process: a fresh interpreter runs them."""
    env = dict(os.environ, FGDM_ATTN_CROSS_LONG='0')
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-q', '-x', '-m', 'gpu', '-k',
                        'test_attention_long_text_contexts and not general'], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]


# ------------------------------------------------------------------------------------------------------------ networks
def build_engine(cfg, **kw):
    from fgdm_amd.engine import Engine
    e = Engine(cfg, **kw)
    for k, shape in e.param_shapes().items():
        e.load_tensor(k, synth.make_tensor(k, shape))
    e.finalize()
    return e


def test_unet_full_width_vs_reference_goldens_long_context():
    from fgdm_amd import _lib
    g, ga = gold('long_context'), gold('long_context_ac')
    e = build_engine(gi.SD_CFG, use_adapter=True)
    try:
        t = torch.from_numpy(g['t'])
        for tok in li.TOKENS:
            x, ctx = li.x(8), li.ctx(tok)
            eps = e.apply_model(x, t, ctx, flags=_lib.FLAG_USE_ORIGINAL | _lib.FLAG_NO_CONTROL)
            check_net(f'unet forward_original 8x8, {tok} tokens', eps.cpu(), g[f'eps_orig_{tok}'], ga[f'eps_orig_{tok}'])
            eps = e.apply_model(x, t, ctx, flags=_lib.FLAG_NO_CONTROL)
            check_net(f'unet FG-DM adapter 8x8, {tok} tokens', eps.cpu(), g[f'eps_fgdm_{tok}'], ga[f'eps_fgdm_{tok}'])
    finally:
        e.close()


def test_control_ldm_full_width_vs_reference_goldens_long_context():
    from fgdm_amd import models
    g, ga = gold('long_context'), gold('long_context_ac')
    e = build_engine(gi.SD_CFG, use_adapter=False, n_controlnets=1)
    try:
        m = models.ControlLDM(gi.SD_CFG, engine=e, n_controlnets=1)
        cond = {'c_concat': [li.hint(128).cuda()], 'c_crossattn': [li.ctx(231).cuda()]}
        eps = m.apply_model(li.x(16).cuda(), torch.from_numpy(g['t']).cuda(), cond)
        check_net('ControlLDM.apply_model 16x16, 231 tokens', eps.cpu(), g['eps_ctrl_231'], ga['eps_ctrl_231'])
    finally:
        e.close()


@pytest.fixture(scope='module')
def small_engine():
    e = build_engine(gi.SMALL_CFG, n_controlnets=1)
    yield e
    e.close()


def _small_inputs(B=2, H=16):
    x = torch.from_numpy(synth.latents(B, H, H, seed=301)).cuda()
    hint = torch.from_numpy(synth.hint(B, 8 * H, seed=302)).cuda()
    t = torch.tensor([981, 21][:B]).cuda()
    return x, t, hint


def test_crossattn_part_list_equals_joined_tensor(small_engine):
    """c_crossattn = [a, b, c] (three [B, 77, 768]) against the one [B, 231, 768] tensor, bit for bit"""
    from fgdm_amd import models
    m = models.ControlLDM(gi.SMALL_CFG, engine=small_engine, n_controlnets=1)
    x, t, hint = _small_inputs()
    ctx = li.ctx(231).cuda()
    parts = [ctx[:, 77 * i: 77 * (i + 1)].contiguous() for i in range(3)]
    a = m.apply_model(x, t, {'c_concat': [hint], 'c_crossattn': parts}).clone()
    b = m.apply_model(x, t, {'c_concat': [hint], 'c_crossattn': [ctx]}).clone()
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    # ... and the parts matter: another third part, another result
    parts2 = parts[:2] + [li.ctx(77).cuda()]
    assert not torch.equal(m.apply_model(x, t, {'c_concat': [hint], 'c_crossattn': parts2}), a)
    # the joined tensor is built once per part list, so the engine registers it once over a sampling loop
    n0 = small_engine._ctx_policy.registrations
    for _ in range(3):
        assert torch.equal(m.apply_model(x, t, {'c_concat': [hint], 'c_crossattn': parts2}),
                           m.apply_model(x, t, {'c_concat': [hint], 'c_crossattn': parts2}))
    assert small_engine._ctx_policy.registrations <= n0 + 1


def test_cached_context_equals_passed_context_and_count_switches(small_engine):
    e = small_engine
    x, t, hint = _small_inputs()
    e.set_hint(0, hint)
    c231, c77 = li.ctx(231).cuda(), li.ctx(77).cuda()
    assert e.lib.fgdm_set_context_tokens(e.h, 0) < 0 and e.lib.fgdm_set_context_tokens(e.h, -3) < 0      # refused ...
    assert e.lib.fgdm_get_context_tokens(e.h) == e._ctx_tokens                                             # ... and nothing changed
    first77 = e.apply_model(x, t, c77).clone()
    assert e.lib.fgdm_get_context_tokens(e.h) == 77
    cached = [e.apply_model(x, t, c231).clone() for _ in range(3)]      # same tensor object: registered once, then reused
    assert e.lib.fgdm_get_context_tokens(e.h) == 231
    assert torch.equal(cached[0], cached[1]) and torch.equal(cached[0], cached[2])
    e.cache_context = False
    try:
        passed = e.apply_model(x, t, c231).clone()                      # projected from the workspace inside the call
    finally:
        e.cache_context = True
    assert torch.equal(passed, cached[0])
    assert not torch.equal(passed, first77)
    # back to 77 tokens with the SAME tensor object as before the switch: the count change dropped the cached projections
    again77 = e.apply_model(x, t, c77).clone()
    assert e.lib.fgdm_get_context_tokens(e.h) == 77
    assert torch.equal(again77, first77)
    # any count >= 1 is served (general kernels outside the fast kernels' ranges)
    for tok in (1, 50, 300):
        a = e.apply_model(x, t, torch.from_numpy(synth.context(2, seed=310 + tok, tokens=tok)).cuda())
        assert bool(torch.isfinite(a).all()), tok
    assert torch.equal(e.apply_model(x, t, c77), first77)


def test_cfg_pair_prefix_sharing_at_231_tokens(small_engine):
    from fgdm_amd import _lib
    x, t, hint = _small_inputs()
    small_engine.set_hint(0, hint)
    x2, t2 = torch.cat([x, x]), torch.cat([t, t])
    ctx = torch.cat([li.ctx(231) * 0.5, li.ctx(231)]).cuda()
    a = small_engine.apply_model(x2, t2, ctx, control_scales=gi.CTRL_SCALES).clone()
    b = small_engine.apply_model(x2, t2, ctx, control_scales=gi.CTRL_SCALES, flags=_lib.FLAG_CFG_PAIRS)
    assert torch.equal(a, b)
    assert not torch.equal(a[:2], a[2:])


def test_device_ddim_loop_equals_python_loop_at_231_tokens(small_engine):
    from fgdm_amd import _lib, engine as E
    from oracle import schedule
    e = small_engine
    x, _, hint = _small_inputs()
    e.set_hint(0, hint)
    c, uc = li.ctx(231).cuda(), (li.ctx(231) * 0.5).cuda()
    tab = schedule.ddim_tables(schedule.register_schedule()['alphas_cumprod'], 5, 0.0)
    S, scale = 5, 7.5
    out = e.sample_ddim(x, c, uc, scale, tab['timesteps'], tab['alphas'], tab['alphas_prev'], tab['sqrt_one_minus_alphas'])
    cur, c_in = x.clone(), torch.cat([uc, c])
    for i in range(S):
        idx = S - 1 - i
        tt = torch.full((4,), int(tab['timesteps'][idx]), dtype=torch.long).cuda()
        e_u, e_c = e.apply_model(torch.cat([cur, cur]), tt, c_in).chunk(2)
        cur, _ = E.ddim_step(cur.contiguous(), e_c.contiguous(), e_u.contiguous(), scale, float(tab['alphas'][idx]),
                             float(tab['alphas_prev'][idx]), 0.0, float(tab['sqrt_one_minus_alphas'][idx]), None, False)
    assert torch.equal(out, cur)
    with pytest.raises(ValueError):       # the device loop runs cat([uncond, cond]) as one batch
        e.sample_ddim(x, c, li.ctx(77).cuda(), scale, tab['timesteps'], tab['alphas'], tab['alphas_prev'],
                      tab['sqrt_one_minus_alphas'])


def test_control_sampler_with_231_token_prompt_and_77_token_negative(small_engine):
    """ControlDDIMSampler.sample with a 231-token c and a 77-token uc: two calls per step (ddim_hacked.py:190-191), equal to
    the hand-combined result"""
    from fgdm_amd import engine as E, models, samplers
    m = models.ControlLDM(gi.SMALL_CFG, engine=small_engine, n_controlnets=1)
    m.control_scales = [0.9] * 13
    x, _, hint = _small_inputs()
    c, uc = li.ctx(231).cuda(), li.ctx(77).cuda()
    cond, ucond = {'c_concat': [hint], 'c_crossattn': [c]}, {'c_concat': [hint], 'c_crossattn': [uc]}
    calls = []
    orig = m.apply_model
    m.apply_model = lambda xx, tt, cc, *a, **k: (calls.append(int(cc['c_crossattn'][0].shape[1])), orig(xx, tt, cc, *a, **k))[1]
    S, scale = 4, 9.0
    smp = samplers.ControlDDIMSampler(m)
    out, _ = smp.sample(S, 2, (4, 16, 16), cond, verbose=False, eta=0.0, x_T=x, unconditional_guidance_scale=scale,
                        unconditional_conditioning=ucond)
    assert calls == [231, 77] * S
    m.apply_model = orig
    cur = x.clone()
    for i in range(S):
        idx = S - 1 - i
        tt = torch.full((2,), int(smp.ddim_timesteps[idx]), dtype=torch.long).cuda()
        e_c, e_u = m.apply_model(cur, tt, cond).clone(), m.apply_model(cur, tt, ucond).clone()
        cur, _ = E.ddim_step(cur.contiguous(), e_c, e_u, scale, float(smp.ddim_alphas[idx]), float(smp.ddim_alphas_prev[idx]),
                             0.0, float(smp.ddim_sqrt_one_minus_alphas[idx]), None, False)
    assert torch.equal(out, cur)


# ------------------------------------------------------------------------------------------------------------ CLIP
@pytest.fixture(scope='module')
def clip_engine():
    e = build_engine(gi.SMALL_CFG, clip=True)
    yield e
    e.close()


def test_clip_skip(clip_engine):
    from oracle import clip as oclip
    ids = gi.clip_ids()
    z = clip_engine.clip_encode(ids)
    for skip in (0, 1):
        assert torch.equal(clip_engine.clip_encode(ids, clip_skip=skip), z), skip
    z2 = clip_engine.clip_encode(ids, clip_skip=2)
    assert not torch.equal(z2, z)
    # final_layer_norm(hidden_states[-2]) = the model with one layer fewer (text_encode ends in the final LayerNorm)
    p = params(oclip.param_shapes())
    with torch.no_grad():
        want = oclip.text_encode(p, ids, cfg=dict(oclip.SD_CLIP, num_hidden_layers=oclip.SD_CLIP['num_hidden_layers'] - 1))
    tol = net_tol(relerr(gold('clip_ac')['z'].astype('float32'), gold('clip')['z']))      # the existing CLIP test's tolerance
    assert report('clip text encoder clip_skip=2 vs oracle', relerr(z2.cpu(), want), tol) < tol
    with pytest.raises(RuntimeError):
        clip_engine.clip_encode(ids, clip_skip=99)


def test_chunked_encoding_equals_three_separate_encodes(clip_engine):
    from fgdm_amd import hack, models
    raws = [li.raw_tokens(n) for n in (10, 151, 300)]
    m = models.LatentDiffusion(engine=clip_engine, use_adapter=False)
    hack.hack_everything(clip_skip=2, model=m)
    m.raw_tokenizer = lambda prompts: raws[:len(prompts)]
    z = m.get_learned_conditioning(['a', 'b', 'c'])
    assert tuple(z.shape) == (3, 231, 768)
    ids = hack.chunk_ids(raws)
    side = torch.cat([clip_engine.clip_encode(ids[:, f], clip_skip=2) for f in range(3)], 1)
    assert torch.equal(z, side)
