"""SD-2.1-base style networks (a fixed head width, nn.Linear proj_in / proj_out, a 1024-wide context) without a GPU: the config
plumbing accepts them and still refuses what the engine does not run, the parameter table equals the reference's state dict
(tests/golden/param_keys_sd21.json, written by tools/make_goldens_sd21.py from the reference's modules), and the d = 64 dispatch
mirror agrees with the case table the GPU test runs."""
import ctypes as C
import json
import os

import pytest

import attention_dispatch as AD
import attention_dispatch_d64 as AD64
import sd21_inputs as si
from common import GOLD
from fgdm_amd import _lib, config, engine as eng, models

UNET = 'ldm.modules.diffusionmodules.openaimodel.UNetModel'
SD21_NODE_PARAMS = dict(image_size=32, in_channels=4, out_channels=4, model_channels=320, attention_resolutions=[4, 2, 1],
                        num_res_blocks=2, channel_mult=[1, 2, 4, 4], num_head_channels=64, use_spatial_transformer=True,
                        use_linear_in_transformer=True, transformer_depth=1, context_dim=1024, legacy=False, use_checkpoint=True)


def test_unet_params_accepts_the_sd2_node():
    kind, cfg, _ = config.unet_params({'target': UNET, 'params': SD21_NODE_PARAMS})
    assert kind == 'unet'
    assert cfg['num_head_channels'] == 64 and cfg['num_heads'] == -1 and cfg['use_linear_in_transformer'] is True
    assert cfg['context_dim'] == 1024
    c = eng.make_config({'target': UNET, 'params': SD21_NODE_PARAMS})
    assert (c.num_head_channels, c.use_linear_in_transformer, c.num_heads, c.context_dim) == (64, 1, -1, 1024)
    # an explicit num_heads = -1 next to the head width is the reference's own default, not "both set"
    assert config.unet_params(dict(SD21_NODE_PARAMS, num_heads=-1))[1] == cfg
    # what unet_params yields goes back in unchanged (models hand it to the engine as `cfg`)
    assert config.unet_params(cfg)[1] == cfg
    # an SD-v1 node yields the dict it always did: the new fields appear only when set
    v1 = config.unet_params(dict(SD21_NODE_PARAMS, num_head_channels=-1, num_heads=8, use_linear_in_transformer=False, context_dim=768))[1]
    assert 'num_head_channels' not in v1 and 'use_linear_in_transformer' not in v1 and v1['num_heads'] == 8


@pytest.mark.parametrize('bad', [dict(num_heads=8),                               # both set
                                 dict(num_head_channels=-1),                      # neither
                                 dict(num_head_channels=48),                      # does not divide 320
                                 dict(num_head_channels=20),                      # not a multiple of 8
                                 dict(parameterization='v'),
                                 dict(transformer_depth=2)], ids=lambda b: ','.join(f'{k}={v}' for k, v in b.items()))
def test_unet_params_still_refuses(bad):
    with pytest.raises(NotImplementedError) as ei:
        config.unet_params({'target': UNET, 'params': dict(SD21_NODE_PARAMS, **bad)})
    assert next(iter(bad)).split('_')[0] in str(ei.value)          # refused by name


def test_v_prediction_and_openclip_refusals_name_the_limit():
    with pytest.raises(NotImplementedError, match='v-prediction'):
        models.LatentDiffusion(unet_config=SD21_NODE_PARAMS, parameterization='v', engine=object())
    with pytest.raises(NotImplementedError, match='OpenCLIP'):
        models.LatentDiffusion.engine_args(unet_config=SD21_NODE_PARAMS, use_adapter=False,
                                           cond_stage_config={'target': 'ldm.modules.encoders.modules.FrozenOpenCLIPEmbedder'})


def test_engine_args_and_controlnet_twin_check():
    a = models.ControlLDM.engine_args(unet_config=si.SD21_SMALL, control_stage_config=dict(si.SD21_SMALL, hint_channels=3))
    assert a['cfg']['num_head_channels'] == 64 and a['cfg']['use_linear_in_transformer'] is True and a['n_controlnets'] == 1
    for other in (dict(si.SD21_SMALL, use_linear_in_transformer=False), dict(si.SD21_SMALL, num_head_channels=-1, num_heads=8),
                  dict(si.SD21_SMALL, num_head_channels=32)):
        with pytest.raises(NotImplementedError, match='matching unet_config'):
            models.ControlLDM.engine_args(unet_config=si.SD21_SMALL, control_stage_config=dict(other, hint_channels=3))
    import golden_inputs as gi                # an SD-v1 UNet with an SD-2 twin, and the other way round
    with pytest.raises(NotImplementedError, match='matching unet_config'):
        models.ControlLDM.engine_args(unet_config=gi.SMALL_CFG, control_stage_config=dict(si.SD21_SMALL, context_dim=768, hint_channels=3))


def test_config_struct_appends_the_two_fields():
    """include/fgdm.h: reserved0 at 204 (the old struct's tail padding), the new fields behind the whole 208-byte struct"""
    c2 = _lib.FgdmConfig2
    assert issubclass(c2, _lib.FgdmConfig) and C.sizeof(_lib.FgdmConfig) == 208
    assert (c2.num_head_channels.offset, c2.use_linear_in_transformer.offset, C.sizeof(c2)) == (208, 212, 216)
    for name, _ in _lib.FgdmConfig._fields_:
        assert getattr(c2, name).offset == getattr(_lib.FgdmConfig, name).offset
    hdr = open(os.path.join(os.path.dirname(GOLD), '..', 'include', 'fgdm.h')).read()
    tail = hdr[hdr.index('int32_t vae_encoder;'):hdr.index('} fgdm_config;')]
    assert tail.index('int32_t reserved0;') < tail.index('int32_t num_head_channels;') < tail.index('int32_t use_linear_in_transformer;')
    import golden_inputs as gi                # zero in both new fields: the SD-v1 table, key for key
    z = eng.make_config(gi.SMALL_CFG)
    want = eng.param_shapes(z)
    z.num_head_channels = 0
    assert eng.param_shapes(z) == want


def _strip(d, prefix):
    return {k[len(prefix):]: list(v) for k, v in d.items() if k.startswith(prefix)}


def test_param_table_matches_reference_keys_sd21():
    ref = json.load(open(os.path.join(GOLD, 'param_keys_sd21.json')))
    got = eng.param_shapes(eng.make_config(si.SD21_SMALL, n_controlnets=1))
    unet, cn = _strip(got, 'model.diffusion_model.'), _strip(got, 'control_model.')
    assert len(unet) + len(cn) == len(got)
    assert list(unet.items()) == list(ref['unet'].items())
    assert list(cn.items()) == list(ref['controlnet'].items())
    proj = [k for k in got if k.endswith(('proj_in.weight', 'proj_out.weight'))]
    assert proj and all(len(got[k]) == 2 for k in proj)
    k2 = [k for k in got if k.endswith('attn2.to_k.weight')]
    assert k2 and all(got[k][1] == 1024 for k in k2)


def test_native_side_refuses_bad_head_settings():
    for kw in (dict(num_heads=8, num_head_channels=64), dict(num_heads=-1, num_head_channels=-1), dict(num_heads=-1, num_head_channels=48),
               dict(num_heads=-1, num_head_channels=20)):
        c = eng.make_config(si.SD21_SMALL)
        c.num_heads, c.num_head_channels = kw['num_heads'], kw['num_head_channels']
        with pytest.raises(ValueError):
            eng.param_shapes(c)
    c = eng.make_config(si.SD21_SMALL)
    c.use_linear_in_transformer = 2
    with pytest.raises(ValueError):
        eng.param_shapes(c)


def test_d64_dispatch_mirror_agrees_with_its_case_table():
    seen = set()
    for T, Tk, want in AD64.D64_CASES:
        assert AD64.expected_kernel_d64(T, Tk, env={}) == want, (T, Tk)
        seen.add((want, (Tk + 31) // 32) if want == AD.LONG_TEXT else want)
    # every kernel family of d = 64 has a case, the text kernel's static (NS = 3), a middle and its largest (NS = 8) form
    assert {AD.TWO_STRAND_32, AD.PING_PONG, AD.TEXT_TOKEN, AD.GENERAL, (AD.LONG_TEXT, 5), (AD.LONG_TEXT, 8)} <= seen
    # the switches move cases the way the launcher's comments say
    assert AD64.expected_kernel_d64(256, 256, env={'FGDM_ATTN_DQ80': '0'}) == AD.PING_PONG
    assert AD64.expected_kernel_d64(256, 256, env={'FGDM_ATTN_DQ80': '0', 'FGDM_ATTN_PP': '0'}) == AD.LONG_TEXT
    assert AD64.expected_kernel_d64(256, 77, env={'FGDM_ATTN_CROSS': '0'}) == AD.GENERAL
    assert AD64.expected_kernel_d64(320, 257, env={'FGDM_ATTN_PP': '0'}) == AD.GENERAL
    # where the rules do not mention the head width, the d = 64 mirror and the older one (d = 40) name the same kernel
    for T, Tk in ((256, 77), (256, 154), (256, 231), (64, 64), (320, 320), (100, 333)):
        assert AD64.expected_kernel_d64(T, Tk, env={}) == AD.expected_kernel(T, Tk, 40, env={}), (T, Tk)
