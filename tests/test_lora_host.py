"""LoRA adapters, the parts that need no GPU (fgdm_amd/lora.py): the kohya name table against the parameter tables of
tests/golden, refusals by name, the alpha / r scale, and the packed-layer grouping of fgdm_weights_update_plan."""
import json
import os

import numpy as np
import pytest
import torch

import golden_inputs as gi
from common import GOLD
from fgdm_amd import engine as eng, lora

U, TE = lora.UNET_PREFIX, lora.TE_PREFIX
# the SD-v1 UNet's SpatialTransformers as kohya (diffusers) names them: (block, index of its attention)
BLOCKS = [(f'down_blocks_{i}', j) for i in range(3) for j in range(2)] + [('mid_block', 0)] + \
         [(f'up_blocks_{i}', j) for i in (1, 2, 3) for j in range(3)]


def test_kohya_table_maps_into_the_parameter_tables():
    unet = json.load(open(os.path.join(GOLD, 'param_keys.json')))['controlled_unet']
    names = [f'lora_unet_{b}_attentions_{j}_{leaf}' for b, j in BLOCKS for leaf in lora.UNET_LEAVES]
    mapped = [lora.kohya_to_ldm(n) for n in names]
    assert len(set(mapped)) == len(names) == 16 * len(lora.UNET_LEAVES) == 16 * 12
    for n, k in zip(names, mapped):
        assert k.startswith(U) and k[len(U):] + '.weight' in unet, (n, k)
    assert lora.kohya_to_ldm('lora_unet_down_blocks_1_attentions_0_transformer_blocks_0_attn1_to_q') == \
        U + 'input_blocks.4.1.transformer_blocks.0.attn1.to_q'
    assert lora.kohya_to_ldm('lora_unet_up_blocks_2_attentions_1_transformer_blocks_0_ff_net_0_proj') == \
        U + 'output_blocks.7.1.transformer_blocks.0.ff.net.0.proj'
    assert lora.kohya_to_ldm('lora_unet_mid_block_attentions_0_proj_out') == U + 'middle_block.1.proj_out'
    clip = json.load(open(os.path.join(GOLD, 'clip_keys.json')))['keys']
    for n in range(12):
        for leaf in lora.TE_LEAVES:
            k = lora.kohya_to_ldm(f'lora_te_text_model_encoder_layers_{n}_{leaf}')
            assert k + '.weight' in clip, k
    assert lora.kohya_to_ldm('lora_te_text_model_encoder_layers_11_self_attn_out_proj') == TE + 'encoder.layers.11.self_attn.out_proj'


@pytest.mark.parametrize('name', ['lora_unet_down_blocks_0_resnets_0_conv1', 'lora_unet_down_blocks_0_attentions_2_proj_in',
                                  'lora_unet_mid_block_attentions_0_transformer_blocks_0_attn3_to_q', 'lora_te_text_model_final_layer_norm',
                                  'lora_te_text_model_encoder_layers_0_mlp_fc3'])
def test_unknown_kohya_names_are_refused_by_name(name):
    with pytest.raises(KeyError, match=name):
        lora.kohya_to_ldm(name)
    z = torch.zeros(4, 4)
    with pytest.raises(KeyError, match=name):
        lora.parse({name + '.lora_down.weight': z, name + '.lora_up.weight': z})


def test_parse_refuses_what_it_cannot_place():
    z = torch.zeros(4, 4)
    with pytest.raises(KeyError, match='some.module.lora_mid.weight'):
        lora.parse({'some.module.lora_mid.weight': z})
    with pytest.raises(KeyError, match="'a.b' has no lora_up.weight"):
        lora.parse({'a.b.lora_down.weight': z, 'a.b.alpha': torch.tensor(4.)})
    p = lora.parse({'a.b.lora_down.weight': z, 'a.b.lora_up.weight': z, 'a.b.alpha': torch.tensor(2.),
                    'lora_unet_mid_block_attentions_0_proj_in.lora_up.weight': z, 'lora_unet_mid_block_attentions_0_proj_in.lora_down.weight': z})
    assert list(p) == ['a.b.weight', U + 'middle_block.1.proj_in.weight']
    assert p['a.b.weight']['alpha'] == 2.0 and p[U + 'middle_block.1.proj_in.weight']['alpha'] is None


def test_effective_scale():
    assert lora.effective_scale(1.0, None, 8) == 1.0
    assert lora.effective_scale(0.75, None, 128) == 0.75
    assert lora.effective_scale(1.0, 4.0, 8) == 0.5
    assert lora.effective_scale(0.6, 16, 4) == 0.6 * 16 / 4
    assert lora.effective_scale(2, 1, 3) == 2.0 * 1.0 / 3.0


@pytest.fixture(scope='module')
def small():
    cfg = eng.make_config(gi.SMALL_CFG, n_controlnets=1, clip=dict(eng.SD_CLIP, num_hidden_layers=2))
    return cfg, eng.param_shapes(cfg)


def test_check_shapes(small):
    _, shapes = small
    t = U + 'input_blocks.1.1.transformer_blocks.0.'
    conv = U + 'input_blocks.1.0.in_layers.2'
    ok = lora.parse({t + 'attn2.to_k.lora_down.weight': torch.zeros(4, 768), t + 'attn2.to_k.lora_up.weight': torch.zeros(320, 4),
                     conv + '.lora_down.weight': torch.zeros(8, 320, 3, 3), conv + '.lora_up.weight': torch.zeros(320, 8, 1, 1)})
    assert lora.check_shapes(ok, shapes) == {t + 'attn2.to_k.weight': (320, 768, 4), conv + '.weight': (320, 2880, 8)}
    bad = lora.parse({conv + '.lora_down.weight': torch.zeros(8, 320, 1, 1), conv + '.lora_up.weight': torch.zeros(320, 8, 3, 3)})
    with pytest.raises(NotImplementedError, match=conv.replace('.', r'\.') + '.*3 x 3'):
        lora.check_shapes(bad, shapes)
    name = 'lora_unet_down_blocks_1_attentions_0_proj_in'        # input_blocks.4.1: not a block of this reduced UNet
    nowhere = lora.parse({name + '.lora_down.weight': torch.zeros(4, 640), name + '.lora_up.weight': torch.zeros(640, 4)})
    with pytest.raises(KeyError, match=name):
        lora.check_shapes(nowhere, shapes)
    wrong = lora.parse({t + 'attn2.to_k.lora_down.weight': torch.zeros(4, 320), t + 'attn2.to_k.lora_up.weight': torch.zeros(320, 4)})
    with pytest.raises(ValueError, match='attn2.to_k'):
        lora.check_shapes(wrong, shapes)


def test_update_plan_groups_what_is_packed_together(small):
    cfg, shapes = small
    wb = lambda *pres: tuple(p + s for p in pres for s in ('.weight', '.bias'))
    t = U + 'middle_block.1.transformer_blocks.0.'
    qkv = (t + 'attn1.to_q.weight', t + 'attn1.to_k.weight', t + 'attn1.to_v.weight') + wb(t + 'norm1')
    for touched in (t + 'attn1.to_q.weight', t + 'attn1.to_v.weight', t + 'norm1.bias'):
        assert lora.plan_update(cfg, [touched]) == [qkv]
    assert lora.plan_update(cfg, [t + 'ff.net.0.proj.weight']) == [wb(t + 'ff.net.0.proj', t + 'norm3')]
    assert lora.plan_update(cfg, [t + 'attn2.to_q.weight']) == [(t + 'attn2.to_q.weight',) + wb(t + 'norm2')]
    assert lora.plan_update(cfg, [t + 'attn2.to_k.weight']) == [(t + 'attn2.to_k.weight',)]
    assert lora.plan_update(cfg, [t + 'attn1.to_out.0.weight']) == [wb(t + 'attn1.to_out.0')]
    p = U + 'middle_block.1.proj_in'
    conv = 'control_model.input_blocks.1.0.in_layers.2'
    zero = 'control_model.zero_convs.1.0'
    assert lora.plan_update(cfg, [zero + '.weight', p + '.weight', conv + '.weight']) == [wb(p), wb(conv), wb(zero)]      # traversal order
    # several touched keys of one layer: the layer once
    assert lora.plan_update(cfg, list(qkv[:3]) + [t + 'attn2.to_k.weight']) == [qkv, (t + 'attn2.to_k.weight',)]
    # every emb_layers Linear of a network is one stacked GEMM
    emb = lora.plan_update(cfg, [U + 'input_blocks.1.0.emb_layers.1.weight'])
    want = [k for k in shapes if k.startswith(U) and '.emb_layers.1.' in k]
    assert len(emb) == 1 and sorted(emb[0]) == sorted(want) and len(want) > 2
    # the text tower's stacked projections, biases included
    a = TE + 'encoder.layers.1.self_attn.'
    assert lora.plan_update(cfg, [a + 'k_proj.weight']) == [wb(a + 'q_proj', a + 'k_proj', a + 'v_proj')]
    assert lora.plan_update(cfg, [TE + 'encoder.layers.0.mlp.fc1.weight']) == [wb(TE + 'encoder.layers.0.mlp.fc1')]
    assert lora.plan_update(cfg, []) == []
    with pytest.raises(KeyError, match='no.such.weight'):
        lora.plan_update(cfg, [t + 'attn1.to_q.weight', 'no.such.weight'])
    # every registered key belongs to at least one packed layer
    owned = {k for unit in lora.plan_update(cfg, list(shapes)) for k in unit}
    assert owned == set(shapes)
