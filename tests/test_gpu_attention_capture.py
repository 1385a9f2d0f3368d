"""Cross-attention capture in the engine (fgdm_attention_capture_*, Engine.capture_attention) on the reduced synthetic UNet
(golden_inputs.SMALL_CFG: seven transformer blocks; a 16 x 16 latent gives T = 256 -- the key-resident text kernel -- and T = 64 --
the general one)."""
import pytest
import torch

import golden_inputs as gi
from attention_maps_cases import measure_bound, relerr
from fgdm_amd import synth

pytestmark = pytest.mark.gpu

BLOCK_RULE = 1e-3      # the project's per-block bar against the oracle's fp32 forward pass


@pytest.fixture(scope='module')
def engine():
    from fgdm_amd.engine import Engine
    e = Engine(gi.SMALL_CFG)
    for k, shape in e.param_shapes().items():
        e.load_tensor(k, synth.make_tensor(k, shape))
    e.finalize()
    yield e
    e.close()


def _inputs(B=2, H=16, W=16, seed=900):
    x = torch.from_numpy(synth.latents(B, H, W, seed=seed)).cuda()
    c = torch.from_numpy(synth.context(B, seed=seed + 1)).cuda()
    uc = torch.from_numpy(synth.context(B, seed=seed + 2)).cuda()
    return x, c, uc


def test_eps_keeps_its_bits_and_kernel_ids_come_back(engine):
    x, c, _ = _inputs()
    t = torch.tensor([981, 21]).cuda()
    lib = engine.lib
    off = engine.apply_model(x, t, c).clone()
    kid_off = lib.fgdm_debug_last_attention_kernel()
    assert kid_off == 2                                     # the last attention of the walk: T = 256 against 77 tokens
    with engine.capture_attention(rows='all', mode='last') as cap:
        on = engine.apply_model(x, t, c).clone()
        assert lib.fgdm_debug_last_attention_kernel() == 8  # its capturing twin
        maps = cap.maps()
        assert cap.n_evals == 1
    assert torch.equal(on, off)
    assert sorted(maps) == list(range(7))
    for b, side in zip(range(7), (16, 8, 8, 8, 8, 16, 16)):
        assert maps[b].shape == (2, side, side, 77) and maps[b].dtype == torch.float32
        assert float((maps[b].sum(-1) - 1).abs().max()) < 1e-5
    again = engine.apply_model(x, t, c)
    assert lib.fgdm_debug_last_attention_kernel() == kid_off and torch.equal(again, off)
    with engine.capture_attention(blocks=[1], rows='all', mode='last'):      # only a T = 64 block: the last attention is not captured
        engine.apply_model(x, t, c)
        assert lib.fgdm_debug_last_attention_kernel() == kid_off


def test_maps_against_the_oracles_own_q_and_k(engine, monkeypatch):
    """the oracle's fp32 forward pass with the engine's weights; its attention (oracle/nn.py) hands over every attn2's q and k, from
    which the map is softmax(q k^T d^-1/2).mean(heads) in float64.  The block's input comes from the oracle's pass, not the
    engine's, so the bar is the per-block 1e-3 rule; token selection and the kernel-level bound are covered elsewhere."""
    from common import params
    from oracle import arch, nn as onn
    x, c, _ = _inputs()
    t = torch.tensor([981, 21])
    seen = []
    real = onn.attention

    def spying(p, pre, xx, ctx, heads, fp32_sim=False):
        if pre.endswith('attn2.'):
            q, k = onn._lin(xx, p, pre + 'to_q', bias=False).double(), onn._lin(ctx, p, pre + 'to_k', bias=False).double()
            b, n, cc = q.shape
            d = cc // heads
            qh, kh = (v.reshape(b, v.shape[1], heads, d).permute(0, 2, 1, 3) for v in (q, k))
            seen.append((torch.matmul(qh, kh.transpose(-1, -2)) * d ** -0.5).softmax(-1).mean(1))
        return real(p, pre, xx, ctx, heads, fp32_sim)
    monkeypatch.setattr(onn, 'attention', spying)
    pre = 'model.diffusion_model.'
    p = params(arch.unet_param_shapes(gi.SMALL_CFG, adapter=False), pre)
    onn.unet_forward(p, gi.SMALL_CFG, x.cpu(), t, c.cpu(), prefix=pre)
    assert len(seen) == 7
    tokens = [0, 3, 76, 40]
    with engine.capture_attention(tokens=tokens, rows='all', mode='last') as cap:
        engine.apply_model(x, t.cuda(), c)
        maps = cap.maps()
    _, _, kernel_bound = measure_bound()
    for b in range(7):
        got = maps[b].reshape(2, -1, len(tokens)).cpu()
        err = relerr(got, seen[b][:, :, tokens])
        print(f'block {b}: captured map vs the oracle block {err:.3e} (rule {BLOCK_RULE:.0e}; kernel-level bound {kernel_bound:.2e})')
        assert err < BLOCK_RULE, (b, err)


def _sample(engine, loop, S=4):
    from fgdm_amd import models, samplers
    m = models.LatentDiffusion(gi.SMALL_CFG, engine=engine, use_adapter=False, image_size=16)
    x_T, c, uc = _inputs()
    torch.manual_seed(77)
    with m.capture_attention(blocks=['mid', 16], tokens=[1, 2, 9], rows='cond', mode='sum') as cap:
        out = samplers.DDIMSampler(m, device_loop=loop).sample(S, 2, (4, 16, 16), c, verbose=False, x_T=x_T, unconditional_guidance_scale=7.5,
                                                              unconditional_conditioning=uc)[0]
        n, raw, maps = cap.n_evals, {b: cap.raw(b).clone() for b in cap.blocks}, cap.maps()
        cap.reset()
        torch.cuda.synchronize()
        assert cap.n_evals == 0 and all(not bool(cap.raw(b).any()) for b in cap.blocks)
    return out, n, raw, maps, cap.blocks


def test_sum_over_a_ddim_sampling_per_step_and_device_loop(engine):
    a, b = _sample(engine, False), _sample(engine, True)
    assert a[4] == b[4] == [0, 2, 5, 6]                                  # 'mid' and the 16 x 16 blocks of a 16 x 16 latent
    assert a[1] == b[1] == 4 and torch.equal(a[0], b[0])
    for blk in a[4]:
        side = 8 if blk == 2 else 16
        assert a[3][blk].shape == (2, side, side, 3)                     # rows = 'cond' under CFG: B rows of the 2 B batch
        assert torch.equal(a[2][blk], b[2][blk]) and torch.equal(a[3][blk], b[3][blk])
        assert torch.equal(a[3][blk], a[2][blk].view(2, side, side, 3) / 4)
        assert float(a[2][blk].min()) >= 0 and float(a[2][blk].max()) <= 4.0 + 1e-4


def test_cond_and_uncond_are_the_halves_of_all(engine):
    x, c, uc = _inputs()
    x2, ctx, t = torch.cat([x] * 2), torch.cat([uc, c]), torch.tensor([500] * 4).cuda()
    got = {}
    for rows in ('all', 'cond', 'uncond'):
        with engine.capture_attention(blocks=[0, 1], tokens=[5], rows=rows, mode='last') as cap:
            engine.apply_model(x2, t, ctx)
            got[rows] = cap.maps()
    for b in (0, 1):
        assert got['all'][b].shape[0] == 4 and got['cond'][b].shape[0] == 2
        assert torch.equal(got['uncond'][b], got['all'][b][:2]) and torch.equal(got['cond'][b], got['all'][b][2:])


def test_refusals(engine):
    from fgdm_amd import _lib
    import ctypes as C
    lib, h = engine.lib, engine.h

    def rc(**kw):
        p = _lib.FgdmAttentionCapture()
        p.struct_size, p.block_mask = C.sizeof(p), 1
        tok = kw.pop('tok', None)
        if tok is not None:
            arr = (C.c_int32 * len(tok))(*tok)
            p.tokens, p.n_tokens = C.cast(arr, C.POINTER(C.c_int32)), len(tok)
        for k, v in kw.items():
            setattr(p, k, v)
        r = lib.fgdm_attention_capture_set(h, C.byref(p))
        lib.fgdm_attention_capture_set(h, None)
        return r
    assert rc() == 0
    for bad in (dict(block_mask=0), dict(block_mask=1 << 7), dict(tok=[77]), dict(tok=[-1]), dict(n_tokens=2), dict(n_tokens=78), dict(rows=3),
                dict(mode=2), dict(struct_size=40), dict(struct_size=56), dict(reserved0=1), dict(batch=2), dict(batch=3, latent_h=8, latent_w=8, rows=1)):
        assert rc(**bad) == -1, bad
    engine.set_context_tokens(308)
    try:
        assert rc() == -1 and b'FGDM_ATTENTION_CAPTURE_MAX_KEYS' in lib.fgdm_last_error(h)
    finally:
        engine.set_context_tokens(77)
    assert lib.fgdm_attention_capture_read(h, 0, C.c_void_p(1 << 20), None) == -1      # capture is off: no block is selected
