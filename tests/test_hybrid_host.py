"""Host side of hybrid conditioning (UNets fed cat([x] + c_concat, 1): DiffusionWrapper 'hybrid', ldm/models/diffusion/ddpm.py:
1838-1841), no GPU: the config plumbing and the parameter table for 9 input channels, every refusal by its message, the memo
rule of the model mirror with a stub engine, and the CPU oracle against the reference's goldens (tests/golden/hybrid*.npz,
recorded by tools/make_goldens.py --only hybrid from LatentDiffusion.apply_model)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import golden_inputs as gi
import hybrid_inputs as hi
from common import GOLD, gold, relerr
from fgdm_amd import _lib, engine as eng, models, samplers
from oracle import arch, nn as onn, precision

TOL = 2e-5      # tests/test_oracle_golden.py: fp32 vs fp32, different op order only


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from fgdm_amd import build
        build.build(verbose=False)
    return _lib.load()


def _create_error(lib, config):
    h = C.c_void_p()
    rc = lib.fgdm_create(C.byref(config), 0, C.byref(h))
    assert rc == -1 and not h.value            # FGDM_ERR_ARG from the config check, before any device is touched
    return lib.fgdm_last_error(None).decode()


# ---------------------------------------------------------------------------------------------------------------- config, table
def test_engine_args_hand_nine_channels_through_without_an_adapter():
    for node in (hi.cfg(9), {'target': 'ldm.modules.diffusionmodules.openaimodel.UNetModel', 'params': dict(hi.cfg(9), image_size=32)}):
        args = models.LatentDiffusion.engine_args(unet_config=node)
        c = eng.make_config(**args)
        assert c.in_channels == 9 and c.use_adapter == 0 and c.out_channels == 4
    c = eng.make_config(**models.LatentDiffusion.engine_args(unet_config=hi.cfg(8), use_adapter=False))
    assert c.in_channels == 8 and c.use_adapter == 0
    # four channels: the FG-DM default (an adapter) is what it was
    assert eng.make_config(**models.LatentDiffusion.engine_args(unet_config=gi.SD_CFG)).use_adapter == 1
    assert eng.make_config(**models.LatentDiffusion.engine_args(unet_config=gi.SD_CFG, use_adapter=True)).use_adapter == 1
    assert eng.make_config(**models.LatentDiffusion.engine_args(unet_config=gi.SD_CFG, use_adapter=False)).use_adapter == 0


def test_param_table_accepts_nine_channels(lib):
    """Fails on an engine that takes in_channels == 4 only: the config check in front of the table refused the config."""
    config = eng.make_config(hi.cfg(9))
    assert lib.fgdm_param_count(C.byref(config)) > 0
    got = eng.param_shapes(config)
    assert got['model.diffusion_model.input_blocks.0.0.weight'] == (320, 9, 3, 3)
    assert got['model.diffusion_model.input_blocks.0.0.bias'] == (320,)
    assert got['model.diffusion_model.out.2.weight'] == (4, 320, 3, 3)
    # everything else is the plain SD UNet's table, and the oracle's shapes for the same config
    plain = eng.param_shapes(eng.make_config(gi.SD_CFG))
    assert list(got) == list(plain)
    assert [k for k in got if got[k] != plain[k]] == ['model.diffusion_model.input_blocks.0.0.weight']
    want = arch.unet_param_shapes(hi.cfg(9), adapter=False)
    assert {hi.PREFIX + k: tuple(s) for k, s in want.items()} == dict(got)
    assert eng.param_shapes(eng.make_config(hi.cfg(8)))['model.diffusion_model.input_blocks.0.0.weight'] == (320, 8, 3, 3)
    assert eng.param_shapes(eng.make_config(hi.cfg(32)))['model.diffusion_model.input_blocks.0.0.weight'] == (320, 32, 3, 3)


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_engine_refuses_adapter_controlnets_and_channel_counts_by_message(lib):
    why = _create_error(lib, eng.make_config(hi.cfg(9), use_adapter=True))
    assert 'use_adapter' in why and 'adapter built for 4 channels' in why
    why = _create_error(lib, eng.make_config(hi.cfg(9), n_controlnets=1))
    assert 'ControlNets' in why and 'DiffusionWrapper' in why
    for bad in (3, 33):
        config = eng.make_config(hi.cfg(bad))
        assert '4 <= in_channels <= 32' in _create_error(lib, config)
        with pytest.raises(ValueError):
            eng.param_shapes(config)
    for config in (eng.make_config(hi.cfg(9), use_adapter=True), eng.make_config(hi.cfg(9), n_controlnets=1)):
        with pytest.raises(ValueError):
            eng.param_shapes(config)


def test_set_concat_and_pack_entry_refuse_without_an_engine(lib):
    p, null = C.c_void_p(1 << 20), None
    assert lib.fgdm_set_concat(null, p, 2, 5, 8, 8, null) == -1
    pack = lambda x=p, cc=p, B=2, Bc=2, Cc=5, H=8, W=8, cp=12, out=p: lib.fgdm_op_pack_xcat(x, cc, B, Bc, Cc, H, W, cp, out, null)
    assert pack(x=null) == -1 and pack(cc=null) == -1 and pack(out=null) == -1
    assert pack(cp=8) == -1            # cin_pad < 4 + Cc
    assert pack(cp=14) == -1           # not a multiple of 4
    assert pack(B=3, Bc=2) == -1       # neither B nor B / 2 rows
    assert pack(B=4, Bc=1) == -1
    assert pack(Cc=0, cp=4) == -1 and pack(H=0) == -1 and pack(B=0, Bc=0) == -1


def test_model_refuses_adapter_with_nine_channels():
    with pytest.raises(NotImplementedError, match='adapter takes the 4 latent channels'):
        models.LatentDiffusion.engine_args(unet_config=hi.cfg(9), use_adapter=True)
    with pytest.raises(NotImplementedError, match='adapter takes the 4 latent channels'):
        models.LatentDiffusion.engine_args(unet_config=hi.cfg(9), use_adapter='time')
    with pytest.raises(NotImplementedError, match='adapter takes the 4 latent channels'):
        models.LatentDiffusion.engine_args(unet_config={'target': 'ldm.modules.diffusionmodules.openaimodel.UNetModel',
                                                        'params': dict(hi.cfg(9), use_time_adapter=True)})


@pytest.mark.parametrize('key,why', [('concat', 'WITHOUT a context'), ('adm', 'class embeddings'), (None, 'unconditional UNet'),
                                     ('bogus', 'DiffusionWrapper knows')])
def test_other_conditioning_keys_keep_raising_with_their_reason(key, why):
    with pytest.raises(NotImplementedError, match=why):
        models.LatentDiffusion(engine=StubEngine(), conditioning_key=key)


# ---------------------------------------------------------------------------------------------------------------- routing, memo
class StubEngine:
    """Records the engine methods the model mirror calls (no GPU, no library); set_concat applies the binding's cache rule."""
    has_vae, has_vae_encoder, has_clip, n_controlnets = False, False, False, 0
    device = torch.device('cpu')

    def __init__(self):
        self.calls, self.uploads, self._key = [], [], None

    def set_concat(self, cc):
        key = (id(cc), cc.data_ptr(), cc._version, tuple(cc.shape))
        if self._key is not None and self._key[0] == key:
            return
        self._key = (key, cc)
        self.uploads.append(cc.clone())

    def apply_model(self, x, t, ctx, control_scales=None, flags=0, pcond=None, out=None):
        self.calls.append(('apply_model', tuple(x.shape), tuple(ctx.shape), flags, pcond))
        return torch.zeros_like(x)


def _hybrid():
    return models.LatentDiffusion(engine=StubEngine(), conditioning_key='hybrid')


def test_hybrid_needs_a_dict_cond_and_no_split_input_params():
    m = _hybrid()
    x, t, c = hi.x(), torch.tensor(hi.T), hi.ctx()
    for cond in (c, [c], (c,)):
        with pytest.raises(TypeError, match='dict cond'):
            m.apply_model(x, t, cond)
    for cond in ({'c_crossattn': [c]}, {'c_crossattn': [c], 'c_concat': None}, {'c_concat': [hi.c_concat(5)]},
                 {'c_crossattn': [c], 'c_concat': hi.c_concat(5)}):
        with pytest.raises(TypeError, match='c_concat'):
            m.apply_model(x, t, cond)
    with pytest.raises(ValueError, match='does not fit'):
        m.apply_model(x, t, {'c_crossattn': [c], 'c_concat': [hi.c_concat(5, H=16, W=16)]})
    with pytest.raises(ValueError, match='does not fit'):
        m.apply_model(x, t, {'c_crossattn': [c], 'c_concat': [hi.c_concat(5, B=3)]})
    assert not m.engine.calls and not m.engine.uploads
    m.split_input_params = {'ks': (4, 4), 'stride': (2, 2)}
    with pytest.raises(NotImplementedError, match='split_input_params'):
        m.apply_model(x, t, {'c_crossattn': [c], 'c_concat': [hi.c_concat(5)]})


def test_c_concat_is_uploaded_once_per_tensor_and_version():
    m = _hybrid()
    x, t = hi.x(), torch.tensor(hi.T)
    mask, latent = hi.c_concat(5)[:, :1].contiguous(), hi.c_concat(5)[:, 1:].contiguous()
    cond = {'c_concat': [mask, latent], 'c_crossattn': [hi.ctx()]}
    for _ in range(3):
        m.apply_model(x, t, cond, use_original=True)
    assert len(m.engine.uploads) == 1 and torch.equal(m.engine.uploads[0], hi.c_concat(5))      # torch.cat(c_concat, 1), once
    assert [c[3] for c in m.engine.calls] == [_lib.FLAG_NO_CONTROL | _lib.FLAG_USE_ORIGINAL] * 3
    latent.mul_(0.5)                                                                             # in place: _version moves on
    m.apply_model(x, t, cond)
    assert len(m.engine.uploads) == 2 and torch.equal(m.engine.uploads[1][:, 1:], latent)
    m.apply_model(x, t, cond)
    assert len(m.engine.uploads) == 2
    # a single part is handed over as it is, and once
    one = {'c_concat': [hi.c_concat(5)], 'c_crossattn': [hi.ctx()]}
    m.apply_model(x, t, one)
    m.apply_model(x, t, one)
    assert len(m.engine.uploads) == 3


def test_pair_flag_needs_equal_halves_or_the_half_batch_tensor():
    m = _hybrid()
    xs, ts, c = hi.x(), torch.tensor(hi.T), torch.cat([hi.ctx(), hi.ctx(seed=8)])
    x, t = torch.cat([xs, xs]), torch.cat([ts, ts])
    half = hi.c_concat(5)
    flags = lambda: m.engine.calls[-1][3]
    m.apply_model(x, t, {'c_concat': [half], 'c_crossattn': [c]}, cfg_pairs=True)             # the sampler's half-batch tensor
    assert flags() == _lib.FLAG_NO_CONTROL | _lib.FLAG_CFG_PAIRS
    m.apply_model(x, t, {'c_concat': [torch.cat([half, half])], 'c_crossattn': [c]}, cfg_pairs=True)      # B rows, equal halves
    assert flags() == _lib.FLAG_NO_CONTROL | _lib.FLAG_CFG_PAIRS
    m.apply_model(x, t, {'c_concat': [torch.cat([torch.zeros_like(half), half])], 'c_crossattn': [c]}, cfg_pairs=True)
    assert flags() == _lib.FLAG_NO_CONTROL                                                     # unequal halves: the flag is dropped
    m.apply_model(x, t, {'c_concat': [half], 'c_crossattn': [c]})                              # nobody asked for pairs
    assert flags() == _lib.FLAG_NO_CONTROL


def test_control_sampler_batches_hybrid_conds():
    """ControlDDIMSampler's batched CFG with a hybrid model: the same c_concat in cond and uncond -> the half-batch tensor and the
    pair flag; different ones -> one 2B batch with c_concat concatenated like the contexts, built once, and no pair flag."""
    m = _hybrid()
    s = samplers.ControlDDIMSampler(m)
    cc, c, uc = hi.c_concat(5), hi.ctx(), hi.ctx(seed=8)
    x, t = hi.x(), torch.tensor(hi.T)
    cond = {'c_concat': [cc], 'c_crossattn': [c]}
    for _ in range(2):
        s._eval_pair(x, t, cond, {'c_concat': [cc], 'c_crossattn': [uc]}, 7.5)
    assert [k[1:4] for k in m.engine.calls] == [((4, 4, 8, 8), (4, 77, 768), _lib.FLAG_NO_CONTROL | _lib.FLAG_CFG_PAIRS)] * 2
    assert len(m.engine.uploads) == 1 and torch.equal(m.engine.uploads[0], cc)
    zeros = {'c_concat': [torch.zeros_like(cc)], 'c_crossattn': [uc]}
    for _ in range(2):
        s._eval_pair(x, t, cond, zeros, 7.5)
    assert [k[1:4] for k in m.engine.calls[2:]] == [((4, 4, 8, 8), (4, 77, 768), _lib.FLAG_NO_CONTROL)] * 2
    assert len(m.engine.uploads) == 2 and torch.equal(m.engine.uploads[1], torch.cat([torch.zeros_like(cc), cc]))
    # an equal but distinct uncond tensor (a clone): concatenated too, and the mirror keeps the pair flag for the equal halves
    s._eval_pair(x, t, cond, {'c_concat': [cc.clone()], 'c_crossattn': [uc]}, 7.5)
    assert m.engine.calls[-1][1:4] == ((4, 4, 8, 8), (4, 77, 768), _lib.FLAG_NO_CONTROL | _lib.FLAG_CFG_PAIRS)
    assert len(m.engine.uploads) == 3 and torch.equal(m.engine.uploads[2], torch.cat([cc, cc]))
    # a ControlLDM-style model (not hybrid) keeps the two-call route for different hints
    plain = models.LatentDiffusion(engine=StubEngine(), use_adapter=False)
    assert samplers.ControlDDIMSampler(plain)._batched_cond(zeros, cond) is None


def test_crossattn_model_makes_the_engine_calls_it_made_before():
    """conditioning_key='crossattn': tensor, list and dict conds, with and without the sampler's hints -- the call log of the stub
    engine, which has no set_concat to call."""
    class Plain:
        has_vae, has_vae_encoder, has_clip, n_controlnets = False, False, False, 0
        device = torch.device('cpu')

        def __init__(self):
            self.calls = []

        def apply_model(self, x, t, ctx, control_scales=None, flags=0, pcond=None, out=None):
            self.calls.append((tuple(x.shape), tuple(ctx.shape), flags, pcond))
            return torch.zeros_like(x)

    m = models.LatentDiffusion(engine=Plain(), use_adapter=False)
    assert m.model.conditioning_key == 'crossattn'
    x, t, c = hi.x(), torch.tensor(hi.T), hi.ctx()
    m.apply_model(x, t, c)
    m.apply_model(x, t, [c], use_original=True, cfg_pairs=True)
    m.apply_model(x, t, {'c_crossattn': [c]}, cfg_pairs=True, pcond=x)
    m.apply_model(x, t, {'c_crossattn': [c], 'c_concat': [hi.c_concat(5)]})       # c_concat is not this mode's business
    N, O, P = _lib.FLAG_NO_CONTROL, _lib.FLAG_USE_ORIGINAL, _lib.FLAG_CFG_PAIRS
    # (the third call: x[0] != x[1], so the mirror drops the pair flag for that pcond, as it always did)
    assert [k[:3] for k in m.engine.calls] == [((2, 4, 8, 8), (2, 77, 768), N), ((2, 4, 8, 8), (2, 77, 768), N | O | P),
                                               ((2, 4, 8, 8), (2, 77, 768), N), ((2, 4, 8, 8), (2, 77, 768), N)]
    assert [k[3] is x for k in m.engine.calls] == [False, False, True, False] and m.engine.calls[0][3] is None


# ---------------------------------------------------------------------------------------------------------------- oracle vs goldens
needs_golden = pytest.mark.skipif(not (os.path.exists(os.path.join(GOLD, 'hybrid.npz')) and os.path.exists(os.path.join(GOLD, 'hybrid_ac.npz'))),
                                  reason='tests/golden/hybrid*.npz not recorded')


def _oracle(cin):
    p = hi.params(arch.unet_param_shapes(hi.cfg(cin), adapter=False))
    xc = torch.cat([hi.x(), hi.c_concat(cin - 4)], 1)
    return onn.unet_forward(p, hi.cfg(cin), xc, torch.tensor(hi.T), hi.ctx(), prefix=hi.PREFIX)


@needs_golden
@pytest.mark.parametrize('cin', hi.IN_CHANNELS)
def test_oracle_reproduces_the_reference_goldens(cin):
    g, ga = gold('hybrid'), gold('hybrid_ac')
    assert list(g['t']) == list(hi.T) and g[f'eps{cin}'].shape == (2, 4, 8, 8)
    with torch.no_grad():
        with precision.mode('fp32'):
            y = _oracle(cin)
        with precision.mode('autocast'):
            ya = _oracle(cin)
    e = relerr(y, g[f'eps{cin}'])
    print(f'hybrid in_channels {cin}: oracle[fp32] vs reference fp32 = {e:.3e}; floor |ref_autocast - ref_fp32| = '
          f'{relerr(ga[f"eps{cin}"].astype(np.float32), g[f"eps{cin}"]):.3e}')
    assert e < TOL
    assert torch.equal(ya.float(), torch.from_numpy(ga[f'eps{cin}'].astype(np.float32)))
