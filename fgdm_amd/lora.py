"""LoRA adapters on a finalized engine: W' = W + scale * alpha / r * up @ down for every touched parameter, merged on the device
by the engine's own kernel (fgdm_op_lora_merge) and re-packed in place (fgdm_weights_*, include/fgdm.h).

Key forms: the ldm names directly -- `<param key without .weight>.lora_down.weight`, `.lora_up.weight`, `.alpha` -- and the kohya
names of SD-v1 files (`lora_unet_...`, `lora_te_...`) through the one table below.  Everything up to `plan_update` is pure: no GPU."""
import ctypes as C
import re
from collections import OrderedDict

import numpy as np
import torch

from . import _lib

UNET_PREFIX = 'model.diffusion_model.'
TE_PREFIX = 'cond_stage_model.transformer.text_model.'
SUFFIXES = ('.lora_down.weight', '.lora_up.weight', '.alpha')

# kohya leaf -> ldm leaf, under a SpatialTransformer (`...N.1.`) of the SD-v1 UNet
UNET_LEAVES = OrderedDict(
    [(f'transformer_blocks_0_attn{a}_to_{p}', f'transformer_blocks.0.attn{a}.to_{p}') for a in (1, 2) for p in 'qkv'] +
    [(f'transformer_blocks_0_attn{a}_to_out_0', f'transformer_blocks.0.attn{a}.to_out.0') for a in (1, 2)] +
    [('transformer_blocks_0_ff_net_0_proj', 'transformer_blocks.0.ff.net.0.proj'), ('transformer_blocks_0_ff_net_2', 'transformer_blocks.0.ff.net.2'),
     ('proj_in', 'proj_in'), ('proj_out', 'proj_out')])
# ... and under a layer of the text tower
TE_LEAVES = OrderedDict([(f'self_attn_{p}_proj', f'self_attn.{p}_proj') for p in ('q', 'k', 'v', 'out')] +
                        [('mlp_fc1', 'mlp.fc1'), ('mlp_fc2', 'mlp.fc2')])

_UNET = re.compile(r'^lora_unet_(down_blocks|up_blocks)_(\d+)_attentions_(\d+)_(.+)$')
_MID = re.compile(r'^lora_unet_mid_block_attentions_0_(.+)$')
_TE = re.compile(r'^lora_te_text_model_encoder_layers_(\d+)_(.+)$')


def kohya_to_ldm(module):
    """`lora_unet_down_blocks_1_attentions_0_transformer_blocks_0_attn1_to_q` -> the ldm module name
    `model.diffusion_model.input_blocks.4.1.transformer_blocks.0.attn1.to_q` (SD-v1: two ResBlocks per level, a downsample behind
    each of the first three).  KeyError, naming the module, for anything the table does not hold."""
    m = _UNET.match(module)
    if m:
        place, i, j, leaf = m.group(1), int(m.group(2)), int(m.group(3)), m.group(4)
        block = f'input_blocks.{3 * i + j + 1}.1' if place == 'down_blocks' else f'output_blocks.{3 * i + j}.1'
        if leaf in UNET_LEAVES and j < (2 if place == 'down_blocks' else 3):
            return f'{UNET_PREFIX}{block}.{UNET_LEAVES[leaf]}'
    m = _MID.match(module)
    if m and m.group(1) in UNET_LEAVES:
        return f'{UNET_PREFIX}middle_block.1.{UNET_LEAVES[m.group(1)]}'
    m = _TE.match(module)
    if m and m.group(2) in TE_LEAVES:
        return f'{TE_PREFIX}encoder.layers.{int(m.group(1))}.{TE_LEAVES[m.group(2)]}'
    raise KeyError(f'LoRA module {module!r} is not in the kohya name table (attention, feed-forward and proj_in / proj_out of the '
                   'SD-v1 UNet; attention and MLP projections of the text tower)')


def effective_scale(scale, alpha, r):
    """scale * alpha / r, alpha taken as r when the file carries none"""
    return float(scale) * (float(r) if alpha is None else float(alpha)) / float(r)


def parse(lora_state_dict):
    """{parameter key: dict(module=<name in the file>, down=, up=, alpha=)} in the file's order.  Every key of the file has to be
    one of a module's `.lora_down.weight` / `.lora_up.weight` / `.alpha`, and every module needs both matrices: anything else is
    refused by name, nothing is dropped."""
    mods = OrderedDict()
    for key, v in lora_state_dict.items():
        for suf in SUFFIXES:
            if key.endswith(suf):
                mods.setdefault(key[:-len(suf)], {})[suf] = v
                break
        else:
            raise KeyError(f'LoRA key {key!r}: expected <module>.lora_down.weight, .lora_up.weight or .alpha')
    out = OrderedDict()
    for module, parts in mods.items():
        for suf in SUFFIXES[:2]:
            if suf not in parts:
                raise KeyError(f'LoRA module {module!r} has no {suf[1:]}')
        name = kohya_to_ldm(module) if module.startswith(('lora_unet_', 'lora_te_')) else module
        alpha = parts.get('.alpha')
        out[name + '.weight'] = dict(module=module, down=parts[SUFFIXES[0]], up=parts[SUFFIXES[1]],
                                     alpha=None if alpha is None else float(np.asarray(alpha).reshape(-1)[0]))
    return out


def check_shapes(parsed, shapes):
    """Every parsed entry against the engine's parameter table `shapes`: -> {parameter key: (O, I, r)}, the flattened view the
    merge kernel takes.  KeyError for a module that maps to no registered parameter, NotImplementedError for a lora_up with a
    kernel larger than 1 x 1, ValueError for matrices that do not fit the parameter; each names the module."""
    dims = OrderedDict()
    for key, d in parsed.items():
        if key not in shapes:
            raise KeyError(f'LoRA module {d["module"]!r} maps to {key!r}, which is no parameter of this engine')
        W = tuple(shapes[key])
        O, I = W[0], int(np.prod(W[1:]))
        up, down = tuple(d['up'].shape), tuple(d['down'].shape)
        if len(up) == 4 and up[2:] != (1, 1):
            raise NotImplementedError(f'LoRA module {d["module"]!r}: lora_up with a {up[2]} x {up[3]} kernel (only 1 x 1 is supported)')
        r = down[0]
        if len(up) not in (2, 4) or up[:2] != (O, r) or len(down) not in (2, 4) or int(np.prod(down[1:])) != I or not 1 <= r <= 128:
            raise ValueError(f'LoRA module {d["module"]!r}: lora_up {up} / lora_down {down} do not fit {key} {W} (rank 1..128)')
        dims[key] = (O, I, r)
    return dims


def plan_update(config, keys):
    """The packed layers of an engine built from `config` that own any of `keys`, each as the tuple of ALL parameter keys it is
    packed from (q, k, v and the folded norm of one attention come together): what an update touching `keys` has to supply.
    Pure: fgdm_weights_update_plan needs no GPU.  KeyError for a key the engine does not register."""
    lib = _lib.load()
    keys = [k.encode() for k in keys]
    arr = (C.c_char_p * len(keys))(*keys)
    need = lib.fgdm_weights_update_plan(C.byref(config), arr, len(keys), None, 0)
    if need < 0:
        why = lib.fgdm_last_error(None)
        raise KeyError(f'fgdm_weights_update_plan failed ({need}): {why.decode() if why else ""}')
    buf = C.create_string_buffer(need)
    lib.fgdm_weights_update_plan(C.byref(config), arr, len(keys), buf, need)
    return [tuple(line.split(' ')) for line in buf.value.decode().splitlines()]


def merge_(W, up, down, s):
    """W += s * up @ down in place on the device: fp32 W [O, ...] taken as [O, I], up [O, r(, 1, 1)], down [r, I...]"""
    O, r = up.shape[0], down.shape[0]
    rc = _lib.load().fgdm_op_lora_merge(W.data_ptr(), up.data_ptr(), down.data_ptr(), float(s), O, W.numel() // O, r, W.data_ptr(),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    if rc != 0:
        raise RuntimeError(f'fgdm_op_lora_merge failed: {rc}')
    return W


def load(engine, loaded, lora_state_dict, base_state_dict, scale=1.0):
    """Merge one more adapter into a finalized `engine` that already carries the adapters `loaded` (what earlier calls returned;
    [] for none) and return the new list.  Every parameter of every packed layer the new adapter touches is rebuilt from
    `base_state_dict` with the deltas of all adapters in call order, one tensor at a time on the device, and the layers are
    re-packed in place; their packed bytes from before the first adapter stay in the engine's snapshot (Engine.weights_restore)."""
    parsed = parse(lora_state_dict)
    dims = check_shapes(parsed, engine.param_shapes())
    adapters = list(loaded) + [dict(parsed=parsed, dims=dims, scale=float(scale))]
    need = [k for unit in plan_update(engine.config, list(parsed)) for k in unit]
    need = list(OrderedDict.fromkeys(need))
    for k in need:
        if k not in base_state_dict:
            raise KeyError(f'base_state_dict has no {k!r}: it is packed together with a parameter this adapter changes')
    dev = lambda v: torch.as_tensor(np.asarray(v) if not torch.is_tensor(v) else v).detach().to(engine.device, torch.float32).contiguous()
    engine.weights_snapshot(need)
    engine.weights_begin_update()
    for k in need:
        W = dev(base_state_dict[k]).clone()
        for a in adapters:
            if k in a['parsed']:
                d, (O, I, r) = a['parsed'][k], a['dims'][k]
                merge_(W, dev(d['up']), dev(d['down']), effective_scale(a['scale'], d['alpha'], r))
        engine.weights_update_tensor(k, W)
        del W
    engine.weights_commit_update()
    return adapters
