"""LoRA adapters on the GPU: the merge kernel alone (fgdm_op_lora_merge), and load_lora / unload_lora on a finalized engine.

The yardstick of the engine tests is torch.equal.  Engine A is finalized from base weights and takes the adapter through
model.load_lora; engine B is finalized from host tensors this file merges itself with the same kernel entry, so the packer of both
reads the same fp32 bits and every output has to agree bit for bit.  The reduced synthetic engine of tests/test_gpu_ddim_loop.py
(golden_inputs.SMALL_CFG, one ControlNet) at 8 x 8 latents, B = 2."""
import ctypes as C

import numpy as np
import pytest
import torch

import golden_inputs as gi
from common import relerr
from fgdm_amd import synth
from guarded import guarded_in, guarded_out

pytestmark = pytest.mark.gpu

U, CN, TE = 'model.diffusion_model.', 'control_model.', 'cond_stage_model.transformer.text_model.'
BLOCK_TOL = 1e-3            # the parity tolerance of tests/test_gpu_blocks.py


# ------------------------------------------------------------------------------------------------------------ the kernel alone
def fma32(a, b, c):
    """fmaf(a, b, c) of float32 arrays, exactly: the product of two float32 is exact in float64; the float64 sum is made
    round-to-odd (TwoSum gives its error; an inexact even result moves to its odd neighbour), which a second rounding to
    float32 cannot get wrong (53 >= 2 * 24 + 2)."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = np.broadcast_to(c.astype(np.float64), p.shape)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    bits = s.copy().view(np.int64)
    fix = (err != 0) & ((bits & 1) == 0)
    away = (err > 0) == (s > 0)          # the exact sum lies farther from zero than s
    bits += np.where(fix, np.where(away, 1, -1), 0)
    return bits.view(np.float64).astype(np.float32)


def merge_ref(W, up, down, s):
    acc = np.zeros_like(W)
    for k in range(up.shape[1]):
        acc = fma32(up[:, k:k + 1], down[k:k + 1, :], acc)
    return fma32(np.float32(s) * np.ones_like(W), acc, W)


def test_fma32_emulation_is_exact():
    """against Python's exact rational arithmetic on inputs that provoke double rounding"""
    from fractions import Fraction
    rng = np.random.default_rng(5)
    a = rng.standard_normal(4000).astype(np.float32)
    b = rng.standard_normal(4000).astype(np.float32)
    c = (rng.standard_normal(4000) * np.exp2(rng.integers(-30, 30, 4000))).astype(np.float32)
    a[:4] = [1 + 2 ** -23, 1 + 2 ** -12, 3, 1 - 2 ** -24]
    b[:4] = [1 + 2 ** -23, 1 + 2 ** -12, 2 ** -25, 1 + 2 ** -23]
    c[:4] = [2 ** -47, 2 ** 24, 1, -1]
    got = fma32(a, b, c)
    for i in range(a.size):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = np.float32(float(exact))                    # float(Fraction) rounds correctly to float64 ...
        # ... so decide float32 exactly: the nearer of the two float32 neighbours of the exact value, ties to even
        cand = sorted({np.nextafter(lo, np.float32(-np.inf)), lo, np.nextafter(lo, np.float32(np.inf))}, key=float)
        best = min(cand, key=lambda v: (abs(Fraction(float(v)) - exact), int(np.float32(v).view(np.int32)) & 1))
        assert got[i] == best, (i, a[i], b[i], c[i], got[i], best)


@pytest.mark.parametrize('O,I,r', [(64, 64, 1), (320, 320, 4), (65, 192, 128), (320, 2880, 8)])
def test_merge_kernel_bits_and_bound(O, I, r):
    from fgdm_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(O * 7 + I + r)
    W = (rng.standard_normal((O, I)) * 0.05).astype(np.float32)
    up = (rng.standard_normal((O, r)) * 0.3).astype(np.float32)
    down = (rng.standard_normal((r, I)) * 0.3).astype(np.float32)
    s = 0.7 * 3 / r if r > 1 else -1.25
    dW, dup, ddown = (guarded_in(torch.from_numpy(v)) for v in (W, up, down))
    out = guarded_out((O, I), torch.float32)
    rc = lib.fgdm_op_lora_merge(dW.data_ptr(), dup.data_ptr(), ddown.data_ptr(), s, O, I, r, out.data_ptr(), None)
    assert rc == 0
    torch.cuda.synchronize()
    got = out.check().cpu().numpy()
    ref = merge_ref(W, up, down, s)
    assert np.array_equal(got.view(np.int32), ref.view(np.int32)), int((got != ref).sum())
    s32 = float(np.float32(s))
    exact = W.astype(np.float64) + s32 * (up.astype(np.float64) @ down.astype(np.float64))
    mag = np.abs(W).astype(np.float64) + abs(s32) * (np.abs(up).astype(np.float64) @ np.abs(down).astype(np.float64))
    assert np.all(np.abs(got.astype(np.float64) - exact) <= (r + 2) * 2.0 ** -24 * mag)
    # in place (out = W), as fgdm_amd/lora.py calls it: the same bits
    rc = lib.fgdm_op_lora_merge(dW.data_ptr(), dup.data_ptr(), ddown.data_ptr(), s, O, I, r, dW.data_ptr(), None)
    assert rc == 0 and torch.equal(dW.cpu(), torch.from_numpy(ref))


def test_merge_entry_refuses_bad_arguments():
    from fgdm_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(1 << 20)
    call = lambda W=p, up=p, down=p, O=64, I=64, r=4, out=p: lib.fgdm_op_lora_merge(W, up, down, 1.0, O, I, r, out, None)
    for bad in (dict(W=None), dict(up=None), dict(down=None), dict(out=None), dict(O=0), dict(I=0), dict(r=0), dict(r=129)):
        assert call(**bad) == -1, bad


# ------------------------------------------------------------------------------------------------------------ engines
@pytest.fixture(scope='module')
def shapes():
    from fgdm_amd import engine as eng
    return eng.param_shapes(eng.make_config(gi.SMALL_CFG, n_controlnets=1))


@pytest.fixture(scope='module')
def base_sd(shapes):
    return {k: synth.make_tensor(k, s) for k, s in shapes.items()}


def _engine(sd, finalize=True, **kw):
    from fgdm_amd.engine import Engine
    e = Engine(gi.SMALL_CFG, **kw)
    for k in e.param_shapes():
        e.load_tensor(k, sd[k])
    if finalize:
        e.finalize()
    return e


def _cldm(engine):
    from fgdm_amd import models
    m = models.ControlLDM(gi.SMALL_CFG, engine=engine, n_controlnets=1)
    m.control_scales = [0.9] * 13
    return m


@pytest.fixture(scope='module')
def engine_a(base_sd):
    e = _engine(base_sd, n_controlnets=1)
    yield e
    e.close()


@pytest.fixture()
def model_a(engine_a):
    m = _cldm(engine_a)
    yield m
    m.unload_lora()
    assert engine_a.weights_snapshot_bytes() == 0


@pytest.fixture(scope='module')
def inputs():
    B, H = 2, 8
    x = torch.from_numpy(synth.latents(B, H, H, seed=910)).cuda()
    c = torch.from_numpy(synth.context(B, seed=911)).cuda()
    uc = torch.from_numpy(synth.context(B, seed=912)).cuda()
    hint = torch.from_numpy(synth.hint(B, res=8 * H, seed=913)).cuda()
    t = torch.tensor([981, 21]).cuda()
    return x, t, c, uc, hint


def _apply(m, inputs):
    x, t, c, _, hint = inputs
    out = m.apply_model(x, t, {'c_concat': [hint], 'c_crossattn': [c]}).clone()
    assert bool(torch.isfinite(out).all())
    return out


def _ddim3(m, inputs, loop):
    """three deterministic DDIM steps with classifier-free guidance: the device loop, or the per-step route"""
    from fgdm_amd import samplers
    x, _, c, uc, hint = inputs
    s = samplers.ControlDDIMSampler(m, device_loop=loop)
    s.make_schedule(5, ddim_eta=0.0, verbose=False)
    return s.decode(x, {'c_concat': [hint], 'c_crossattn': [c]}, 3, unconditional_guidance_scale=6.0,
                    unconditional_conditioning={'c_concat': [hint], 'c_crossattn': [uc]}).clone()


T1, TM = 'input_blocks.1.1.transformer_blocks.0.', 'middle_block.1.transformer_blocks.0.'
ATTN = [U + T1 + f'attn{a}.to_{p}.weight' for a in (1, 2) for p in 'qkv'] + [U + T1 + 'attn1.to_out.0.weight',
        U + TM + 'attn1.to_q.weight', U + TM + 'attn2.to_k.weight', U + TM + 'attn2.to_out.0.weight',
        U + 'output_blocks.0.1.transformer_blocks.0.attn1.to_v.weight']
# ... some of them under the names a kohya file gives them
KOHYA = {U + T1 + 'attn1.to_q.weight': 'lora_unet_down_blocks_0_attentions_0_transformer_blocks_0_attn1_to_q',
         U + TM + 'attn2.to_k.weight': 'lora_unet_mid_block_attentions_0_transformer_blocks_0_attn2_to_k',
         U + TM + 'ff.net.0.proj.weight': 'lora_unet_mid_block_attentions_0_transformer_blocks_0_ff_net_0_proj',
         U + 'output_blocks.0.1.proj_out.weight': 'lora_unet_up_blocks_0_attentions_0_proj_out'}
BROAD = ATTN[:4] + [U + TM + 'ff.net.0.proj.weight', U + T1 + 'ff.net.2.weight', U + 'input_blocks.1.1.proj_in.weight',
                    U + 'output_blocks.0.1.proj_out.weight', U + 'input_blocks.1.0.in_layers.2.weight',
                    U + 'output_blocks.1.2.conv.weight', U + 'middle_block.0.emb_layers.1.weight']
CONTROL = [CN + T1 + 'attn1.to_k.weight', CN + T1 + 'attn2.to_v.weight', CN + TM + 'ff.net.0.proj.weight', CN + 'zero_convs.1.0.weight',
           CN + 'middle_block_out.0.weight', CN + 'input_hint_block.2.weight', CN + 'input_blocks.3.0.skip_connection.weight']
CASES = {'attention': (ATTN, 4, 2.0, 1.0), 'broad': (BROAD, 8, None, 0.8), 'controlnet': (CONTROL, 5, 10.0, 1.0)}


def make_adapter(shapes, keys, r, alpha, seed, names=KOHYA):
    """a synthetic adapter as a LoRA file holds it, and {parameter key: (down, up, alpha)} for this file's own merge"""
    sd, spec = {}, {}
    for n, key in enumerate(keys):
        W = tuple(shapes[key])
        rng = np.random.default_rng(seed * 1000 + n)
        down = torch.from_numpy((rng.standard_normal((r,) + W[1:]) * 0.08).astype(np.float32))
        up = torch.from_numpy((rng.standard_normal((W[0], r) + (1, 1) * (len(W) == 4)) * 0.08).astype(np.float32))
        name = names.get(key, key[:-len('.weight')])
        sd[name + '.lora_down.weight'], sd[name + '.lora_up.weight'] = down, up
        if alpha is not None:
            sd[name + '.alpha'] = torch.tensor(float(alpha))
        spec[key] = (down, up, alpha)
    return sd, spec


def merged_sd(base_sd, adapters):
    """base_sd with the adapters [(spec, scale)] merged in call order by the kernel entry: what engine B is finalized from"""
    from fgdm_amd import _lib
    lib = _lib.load()
    sd = dict(base_sd)
    for spec, scale in adapters:
        for key, (down, up, alpha) in spec.items():
            W = torch.as_tensor(sd[key]).cuda().contiguous()
            O, r = up.shape[0], down.shape[0]
            s = scale * (r if alpha is None else alpha) / r
            out = torch.empty_like(W)
            assert lib.fgdm_op_lora_merge(W.data_ptr(), up.cuda().data_ptr(), down.cuda().data_ptr(), s, O, W.numel() // O, r,
                                          out.data_ptr(), None) == 0
            torch.cuda.synchronize()
            sd[key] = out.cpu().numpy()
    return sd


_refs = {}


def reference(name, shapes, base_sd, inputs):
    """the adapter of CASES[name], and what engine B -- finalized from the merged weights -- computes; made once per module"""
    if name not in _refs:
        keys, r, alpha, scale = CASES[name]
        lora_sd, spec = make_adapter(shapes, keys, r, alpha, seed=len(keys))
        b = _engine(merged_sd(base_sd, [(spec, scale)]), n_controlnets=1)
        mb = _cldm(b)
        _refs[name] = dict(lora=lora_sd, spec=spec, scale=scale, out=_apply(mb, inputs),
                           ddim=_ddim3(mb, inputs, loop=False) if name == 'controlnet' else None)
        b.close()
    return _refs[name]


@pytest.fixture(scope='module')
def base_out(engine_a, inputs):
    return _apply(_cldm(engine_a), inputs)


@pytest.mark.parametrize('name', list(CASES))
def test_merge_equals_rebuild(model_a, base_out, shapes, base_sd, inputs, name):
    """... with the context registered and the hint set BEFORE the load: the stale text K / V^T and hint features must not be
    reused (the ControlNet adapter changes the hint block, every adapter with attn2.to_k / to_v the text projections)"""
    ref = reference(name, shapes, base_sd, inputs)
    assert torch.equal(_apply(model_a, inputs), base_out)          # registers inputs' context, caches the hint features
    model_a.load_lora(ref['lora'], base_sd, scale=ref['scale'])
    assert model_a.engine.weights_snapshot_bytes() > 0
    got = _apply(model_a, inputs)
    assert torch.equal(got, ref['out'])
    assert relerr(got, base_out) > BLOCK_TOL


def test_device_loop_after_load_equals_per_step_route_of_rebuild(model_a, shapes, base_sd, inputs):
    ref = reference('controlnet', shapes, base_sd, inputs)
    before = _ddim3(model_a, inputs, loop=True)                      # the loop registers its contexts and uses the cached hint
    model_a.load_lora(ref['lora'], base_sd, scale=ref['scale'])
    got = _ddim3(model_a, inputs, loop=True)
    assert torch.equal(got, ref['ddim']) and not torch.equal(got, before)
    assert torch.equal(_ddim3(model_a, inputs, loop=False), ref['ddim'])


def test_load_unload_load(model_a, base_out, shapes, base_sd, inputs):
    ref = reference('broad', shapes, base_sd, inputs)
    model_a.load_lora(ref['lora'], base_sd, scale=ref['scale'])
    first = _apply(model_a, inputs)
    assert relerr(first, base_out) > BLOCK_TOL and torch.equal(first, ref['out'])
    held = model_a.engine.weights_snapshot_bytes()
    assert held > 0
    model_a.unload_lora()
    assert model_a.engine.weights_snapshot_bytes() == 0
    assert torch.equal(_apply(model_a, inputs), base_out)
    model_a.load_lora(ref['lora'], base_sd, scale=ref['scale'])
    assert model_a.engine.weights_snapshot_bytes() == held
    assert torch.equal(_apply(model_a, inputs), first)


def test_second_adapter_merges_on_top(model_a, base_out, shapes, base_sd, inputs):
    """two adapters sharing parameters: the sum from the base with the deltas in call order, and one unload undoes both"""
    one, spec1 = make_adapter(shapes, ATTN, 4, 2.0, seed=31)
    two, spec2 = make_adapter(shapes, BROAD, 2, None, seed=32)
    b = _engine(merged_sd(base_sd, [(spec1, 0.7), (spec2, 1.1)]), n_controlnets=1)
    want = _apply(_cldm(b), inputs)
    b.close()
    model_a.load_lora(one, base_sd, scale=0.7)
    model_a.load_lora(two, base_sd, scale=1.1)
    assert torch.equal(_apply(model_a, inputs), want)
    model_a.unload_lora()
    assert torch.equal(_apply(model_a, inputs), base_out)


def test_refusals_leave_the_engine_as_it_was(model_a, base_out, shapes, base_sd, inputs):
    e = model_a.engine
    q = U + T1 + 'attn1.to_q.weight'
    dev = lambda k: torch.as_tensor(base_sd[k]).cuda() * 1.5
    e.weights_begin_update()                                        # a partly supplied packed layer: q without k, v and norm1
    e.weights_update_tensor(q, dev(q))
    with pytest.raises(RuntimeError, match=r'partly supplied packed layer.*attn1\.to_k\.weight'):
        e.weights_commit_update()
    assert torch.equal(_apply(model_a, inputs), base_out)
    with pytest.raises(RuntimeError, match='fgdm_weights_begin_update has not been called'):      # the refused commit ended the update
        e.weights_update_tensor(q, dev(q))
    e.weights_begin_update()
    with pytest.raises(RuntimeError, match='shape mismatch for ' + q.replace('.', r'\.')):
        e.weights_update_tensor(q, dev(q)[:, :64])
    with pytest.raises(RuntimeError, match='rank mismatch'):
        e.weights_update_tensor(q, dev(q)[None])
    with pytest.raises(RuntimeError, match='unknown parameter key: no.such.weight'):
        e.weights_update_tensor('no.such.weight', dev(q))
    e.weights_commit_update()                                       # nothing was accepted: nothing changes
    with pytest.raises(RuntimeError, match='unknown parameter key'):
        e.weights_snapshot([q, 'no.such.weight'])
    assert e.weights_snapshot_bytes() == 0
    with pytest.raises(RuntimeError, match='no weight snapshot'):
        e.weights_restore()
    assert torch.equal(_apply(model_a, inputs), base_out)
    # through load_lora: a module that maps to no parameter, a 3 x 3 lora_up, a base state dict that lacks a partner key
    ad, _ = make_adapter(shapes, ATTN[:1], 4, None, seed=40, names={})
    with pytest.raises(KeyError, match='bogus.layer'):
        model_a.load_lora(dict(ad, **{'bogus.layer.lora_down.weight': torch.zeros(4, 8), 'bogus.layer.lora_up.weight': torch.zeros(8, 4)}), base_sd)
    conv = U + 'input_blocks.1.0.in_layers.2'
    with pytest.raises(NotImplementedError, match='3 x 3'):
        model_a.load_lora({conv + '.lora_down.weight': torch.zeros(4, 320, 1, 1), conv + '.lora_up.weight': torch.zeros(320, 4, 3, 3)}, base_sd)
    with pytest.raises(KeyError, match=r'attn1\.to_v\.weight'):
        model_a.load_lora(ad, {k: v for k, v in base_sd.items() if k != U + T1 + 'attn1.to_v.weight'})
    assert e.weights_snapshot_bytes() == 0
    assert torch.equal(_apply(model_a, inputs), base_out)


def test_update_before_finalize_is_refused(base_sd, base_out, inputs):
    e = _engine(base_sd, finalize=False, n_controlnets=1)
    q = U + T1 + 'attn1.to_q.weight'
    for call in (e.weights_begin_update, lambda: e.weights_update_tensor(q, torch.as_tensor(base_sd[q]).cuda()), e.weights_commit_update,
                 lambda: e.weights_snapshot([q]), e.weights_restore):
        with pytest.raises(RuntimeError, match='not finalized'):
            call()
    e.finalize()
    assert torch.equal(_apply(_cldm(e), inputs), base_out)
    e.close()


def test_text_tower_adapter(base_sd):
    """get_learned_conditioning of an engine with a (two-layer) text tower: merge equals rebuild, and unload restores"""
    from fgdm_amd import engine as eng, models
    clip = dict(eng.SD_CLIP, num_hidden_layers=2, vocab_size=1024)
    shapes = eng.param_shapes(eng.make_config(gi.SMALL_CFG, clip=clip))
    sd = {k: base_sd[k] if k in base_sd else synth.make_tensor(k, s) for k, s in shapes.items()}
    L = TE + 'encoder.layers.'
    keys = [L + '0.self_attn.q_proj.weight', L + '0.self_attn.out_proj.weight', L + '1.self_attn.v_proj.weight', L + '1.mlp.fc1.weight',
            L + '0.mlp.fc2.weight']
    names = {L + '0.self_attn.q_proj.weight': 'lora_te_text_model_encoder_layers_0_self_attn_q_proj',
             L + '1.mlp.fc1.weight': 'lora_te_text_model_encoder_layers_1_mlp_fc1',
             L + '0.mlp.fc2.weight': 'lora_te_text_model_encoder_layers_0_mlp_fc2'}
    lora_sd, spec = make_adapter(shapes, keys, 6, 3.0, seed=50, names=names)
    ids = torch.from_numpy(np.random.default_rng(51).integers(0, 1024, size=(2, 77)))
    b = _engine(merged_sd(sd, [(spec, 0.9)]), clip=clip)
    want = models.LatentDiffusion(gi.SMALL_CFG, engine=b, use_adapter=False).get_learned_conditioning(ids).clone()
    b.close()
    a = _engine(sd, clip=clip)
    m = models.LatentDiffusion(gi.SMALL_CFG, engine=a, use_adapter=False)
    base = m.get_learned_conditioning(ids).clone()
    m.load_lora(lora_sd, sd, scale=0.9)
    got = m.get_learned_conditioning(ids).clone()
    assert torch.equal(got, want) and bool(torch.isfinite(got).all()) and relerr(got, base) > BLOCK_TOL
    m.unload_lora()
    assert torch.equal(m.get_learned_conditioning(ids), base)
    a.close()
