"""CPU-side checks of the C-ABI library: it loads, exports every symbol include/fgdm.h declares, and the
engine's parameter table matches the reference state_dict keys/shapes (golden param_keys.json).
No compute calls: these run without a GPU."""
import json
import os
import re

import pytest

import golden_inputs as gi
from common import GOLD
from fgdm_amd import _lib, engine as eng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from fgdm_amd import build
        build.build(verbose=False)
    return _lib.load()


def test_header_symbols_exported(lib):
    hdr = open(os.path.join(ROOT, 'include', 'fgdm.h')).read()
    declared = set(re.findall(r'\b(fgdm_[a-z0-9_]+)\s*\(', hdr))
    assert declared, 'no declarations parsed'
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    for name in declared:
        assert hasattr(lib, name), name


def _strip(d, prefix):
    return {k[len(prefix):]: tuple(v) for k, v in d.items() if k.startswith(prefix)}


def test_param_table_matches_reference_keys(lib):
    ref = json.load(open(os.path.join(GOLD, 'param_keys.json')))
    # FG-DM UNet (with adapter) + one ControlNet
    got = eng.param_shapes(eng.make_config(gi.SD_CFG, use_adapter=True, n_controlnets=1))
    unet = _strip(got, 'model.diffusion_model.')
    assert list(unet.keys()) == list(ref['unet_fgdm'].keys())
    assert all(tuple(ref['unet_fgdm'][k]) == v for k, v in unet.items())
    cn = _strip(got, 'control_model.')
    assert list(cn.keys()) == list(ref['controlnet'].keys())
    assert all(tuple(ref['controlnet'][k]) == v for k, v in cn.items())
    # TimeAdapter variant (use_time_adapter=True)
    got = eng.param_shapes(eng.make_config(gi.SD_CFG, use_adapter='time'))
    unet = _strip(got, 'model.diffusion_model.')
    assert list(unet.keys()) == list(ref['unet_time_adapter'].keys())
    assert all(tuple(ref['unet_time_adapter'][k]) == v for k, v in unet.items())
    # AdaptUNetModel(num_prompts=3): two further adapters registered right after `adapter`
    got = eng.param_shapes(eng.make_config(gi.SD_CFG, use_adapter=True, num_prompts=3))
    unet = _strip(got, 'model.diffusion_model.')
    assert list(unet.keys()) == list(ref['adapt_unet_3'].keys())
    assert all(tuple(ref['adapt_unet_3'][k]) == v for k, v in unet.items())
    # plain SD UNet (= ControlledUnetModel keys)
    got = eng.param_shapes(eng.make_config(gi.SD_CFG))
    unet = _strip(got, 'model.diffusion_model.')
    assert list(unet.keys()) == list(ref['controlled_unet'].keys())
    # reduced-depth config
    got = eng.param_shapes(eng.make_config(gi.SMALL_CFG, n_controlnets=1))
    assert list(_strip(got, 'model.diffusion_model.').keys()) == list(ref['unet_small'].keys())
    assert list(_strip(got, 'control_model.').keys()) == list(ref['controlnet_small'].keys())
    # first-stage decoder keys follow the UNet / ControlNet tables (AutoencoderKL decoder.* + post_quant_conv.*)
    got = eng.param_shapes(eng.make_config(gi.SD_CFG, vae=True))
    vae = {k: v for k, v in got.items() if k.startswith('first_stage_model.')}
    assert list(vae.keys()) == list(ref['vae_decoder'].keys())
    assert all(tuple(ref['vae_decoder'][k]) == v for k, v in vae.items())
    assert list(got.keys())[-len(vae):] == list(vae.keys())
    # text-encoder keys (transformers.CLIPTextModel under the checkpoints' prefix) come last
    got = eng.param_shapes(eng.make_config(gi.SD_CFG, vae=True, clip=True))
    ck = json.load(open(os.path.join(GOLD, 'clip_keys.json')))['keys']
    clip = {k: v for k, v in got.items() if k.startswith('cond_stage_model.')}
    assert list(clip.keys()) == list(ck.keys())
    assert all(tuple(ck[k]) == v for k, v in clip.items())
    assert list(got.keys())[-len(clip):] == list(clip.keys())
    # several ControlNets get distinct prefixes
    got = eng.param_shapes(eng.make_config(gi.SD_CFG, n_controlnets=3))
    assert any(k.startswith('control_model_1.') for k in got) and any(k.startswith('control_model_2.') for k in got)


def test_unsupported_configs_are_rejected(lib):
    bad = dict(gi.SD_CFG, model_channels=160)          # not a multiple of 64
    with pytest.raises(ValueError):
        eng.param_shapes(eng.make_config(bad))
    with pytest.raises(ValueError):                     # decoder attention at up levels is not implemented
        eng.make_config(gi.SD_CFG, vae=dict(eng.SD_VAE, attn_resolutions=[32]))
    with pytest.raises(ValueError):                     # decoder width must be a multiple of 64
        eng.param_shapes(eng.make_config(gi.SD_CFG, vae=dict(eng.SD_VAE, ch=96)))
    with pytest.raises(ValueError):                     # extra adapters need the FG-DM adapter
        eng.param_shapes(eng.make_config(gi.SD_CFG, use_adapter=False, num_prompts=2))
    with pytest.raises(ValueError):                     # text encoder: head dim must be 64
        eng.param_shapes(eng.make_config(gi.SD_CFG, clip=dict(eng.SD_CLIP, num_attention_heads=8)))
    with pytest.raises(ValueError):                     # adapter needs the SD-v1 topology
        eng.param_shapes(eng.make_config(gi.SMALL_CFG, use_adapter=True))


def test_narrow_op_entries_refuse_bad_arguments(lib):
    """The diagnostic entries of tests/test_gpu_narrow_ops.py return FGDM_ERR_ARG before any launch (so without a GPU too): the
    pointers below are never dereferenced."""
    import ctypes as C
    p, null = C.c_void_p(1 << 20), None
    # fgdm_op_conv2d with Cin % 64 != 0: ksize 3, C1 == 0, no upsample, stride 1 or 2 only
    conv = lambda C0, x1, C1, ks, stride, up: lib.fgdm_op_conv2d(p, C0, x1, C1, p, p, null, null, 1, 8, 8, 16, ks, stride, up, 0, 1.0, p, null)
    assert conv(4, null, 0, 1, 1, 0) < 0                      # ksize 1
    assert conv(4, p, 4, 3, 1, 0) < 0                         # a concatenated input
    assert conv(4, null, 0, 3, 1, 1) < 0                      # upsample
    assert conv(4, null, 0, 3, _lib.STRIDE2_PAD_BR, 0) < 0    # the encoder's bottom / right padding
    assert conv(4, null, 0, 3, 3, 0) < 0                      # stride 3
    assert conv(96, null, 0, 1, 1, 0) < 0
    assert lib.fgdm_op_conv2d(null, 4, null, 0, p, p, null, null, 1, 8, 8, 16, 3, 1, 0, 0, 1.0, p, null) < 0
    assert lib.fgdm_op_conv2d(p, 4, null, 0, p, p, null, null, 0, 8, 8, 16, 3, 1, 0, 0, 1.0, p, null) < 0
    # fgdm_op_vae_attention: NULL pointers, T % 64 != 0, C % 64 != 0
    for args in ((null, p, p, p), (p, null, p, p), (p, p, null, p), (p, p, p, null)):
        assert lib.fgdm_op_vae_attention(*args, 1, 64, 512, null) < 0
    assert lib.fgdm_op_vae_attention(p, p, p, p, 1, 100, 512, null) < 0
    assert lib.fgdm_op_vae_attention(p, p, p, p, 1, 64, 100, null) < 0
    assert lib.fgdm_op_vae_attention(p, p, p, p, 0, 64, 512, null) < 0
    # the layout / elementwise entries
    assert lib.fgdm_op_softmax_rows(null, p, 4, 64, null) < 0 and lib.fgdm_op_softmax_rows(p, null, 4, 64, null) < 0
    assert lib.fgdm_op_softmax_rows(p, p, 0, 64, null) < 0 and lib.fgdm_op_softmax_rows(p, p, 4, 0, null) < 0
    assert lib.fgdm_op_nchw_to_nhwc(null, p, 1, 3, 64, 4, null) < 0 and lib.fgdm_op_nchw_to_nhwc(p, null, 1, 3, 64, 4, null) < 0
    assert lib.fgdm_op_nchw_to_nhwc(p, p, 1, 4, 64, 3, null) < 0         # Cpad < C
    assert lib.fgdm_op_nhwc_to_nchw(null, p, 1, 4, 64, null) < 0 and lib.fgdm_op_nhwc_to_nchw(p, null, 1, 4, 64, null) < 0
    assert lib.fgdm_op_nhwc_to_nchw(p, p, 1, 4, 0, null) < 0
    assert lib.fgdm_op_avgpool2(null, p, 1, 8, 8, 8, null) < 0 and lib.fgdm_op_avgpool2(p, null, 1, 8, 8, 8, null) < 0
    assert lib.fgdm_op_avgpool2(p, p, 1, 7, 8, 8, null) < 0              # odd H
    assert lib.fgdm_op_avgpool2(p, p, 1, 8, 7, 8, null) < 0              # odd W
    assert lib.fgdm_op_avgpool2(p, p, 1, 8, 8, 12, null) < 0             # C % 8
    assert lib.fgdm_op_transpose_pad(null, p, 1, 77, 320, 128, null) < 0 and lib.fgdm_op_transpose_pad(p, null, 1, 77, 320, 128, null) < 0
    assert lib.fgdm_op_transpose_pad(p, p, 1, 77, 320, 64, null) < 0     # Tkpad < Tk
    assert lib.fgdm_op_timestep_embed(null, null, p, 1, 320, 1, null) < 0 and lib.fgdm_op_timestep_embed(p, null, null, 1, 320, 1, null) < 0
    assert lib.fgdm_op_timestep_embed(p, null, p, 2, 320, 1, null) < 0   # rows_pad < B
    assert lib.fgdm_op_timestep_embed(p, null, p, 1, 321, 1, null) < 0   # odd dim
    assert lib.fgdm_op_add_f16(null, p, p, 8, null) < 0 and lib.fgdm_op_add_f16(p, null, p, 8, null) < 0
    assert lib.fgdm_op_add_f16(p, p, null, 8, null) < 0
    assert lib.fgdm_op_add_f16(p, p, p, 12, null) < 0                    # n % 8
    assert lib.fgdm_op_add_f16(p, p, p, 0, null) < 0


def test_fp32_op_entries_refuse_bad_arguments(lib):
    """The diagnostic entries of tests/test_gpu_fp32_ops.py return FGDM_ERR_ARG before any launch (so without a GPU too): the
    pointers below are never dereferenced."""
    import ctypes as C
    p, null = C.c_void_p(1 << 20), None
    ERR_ARG = -1

    def refuses(fn, good, bad):
        """every argument set that differs from `good` in the named positions is refused"""
        for change in bad:
            args = list(good)
            for i, v in change.items():
                args[i] = v
            assert fn(*args) == ERR_ARG, (fn.__name__, change)

    nulls = lambda *idx: [{i: null} for i in idx]
    nonpos = lambda *idx: [{i: v} for i in idx for v in (0, -1)]
    # ids, tok, pos, out, rows, T, W, vocab, stream
    refuses(lib.fgdm_op_embed_tokens, (p, p, p, p, 154, 77, 768, 1000, null),
            nulls(0, 1, 2, 3) + nonpos(4, 5, 6, 7) + [{6: 4}, {6: 12}, {6: 769}, {6: 772}])           # W % 8 != 0
    # x, rows, C, gamma, beta, eps, out16, out32, stream: exactly one output
    for good in ((p, 5, 768, p, p, 1e-5, p, null, null), (p, 5, 768, p, p, 1e-5, null, p, null)):
        refuses(lib.fgdm_op_layernorm32, good, nulls(0, 3, 4) + nonpos(1, 2) + [{2: 1}, {2: 2}, {2: 767}, {2: 770}]  # C % 4 != 0
                + [{6: p, 7: p}, {6: null, 7: null}])
    # a, b16, y, n, stream
    refuses(lib.fgdm_op_add_f16_to_f32, (p, p, p, 12345, null), nulls(0, 1, 2) + nonpos(3))
    # x, y, n, stream
    refuses(lib.fgdm_op_f32_to_f16, (p, p, 12345, null), nulls(0, 1) + nonpos(2))
    refuses(lib.fgdm_op_silu_f32_to_f16, (p, p, 12345, null), nulls(0, 1) + nonpos(2))
    # z, wb, scale, y, B, HW, stream
    refuses(lib.fgdm_op_vae_prequant, (p, p, 1.0, p, 3, 1000, null), nulls(0, 1, 3) + nonpos(4, 5))
    # h, wb, moments, B, HW, stream
    refuses(lib.fgdm_op_vae_moments, (p, p, p, 3, 1000, null), nulls(0, 1, 2) + nonpos(3, 4))


def test_ln_qkv_entry_refuses_bad_arguments(lib):
    """fgdm_op_ln_qkv (tests/test_gpu_qkv_projection.py) returns FGDM_ERR_ARG before any launch or copy for every refusal
    include/fgdm.h lists (so without a GPU too): the pointers below are never dereferenced."""
    import ctypes as C
    p, null = C.c_void_p(1 << 20), None
    ERR_ARG = -1

    def call(h=p, gamma=p, beta=p, wq=p, wk=p, wv=p, B=2, T=64, Cc=320, Tp=64, fold=1, qk=p, vt=p):
        return lib.fgdm_op_ln_qkv(h, gamma, beta, wq, wk, wv, B, T, Cc, Tp, fold, qk, vt, null)

    for name in ('h', 'wq', 'wk', 'wv', 'qk', 'vt'):
        assert call(**{name: null}) == ERR_ARG, name
    for name in ('B', 'T', 'Cc'):
        for bad in (0, -1):
            assert call(**{name: bad}) == ERR_ARG, (name, bad)
    for bad in (64, 160, 256, 321, 960 + 64):            # C % 320 != 0
        assert call(Cc=bad) == ERR_ARG, bad
    assert call(T=100, Tp=96) == ERR_ARG                 # Tp < T
    assert call(T=64, Tp=63) == ERR_ARG
    assert call(T=100, Tp=100) == ERR_ARG                # Tp % 8 != 0
    assert call(T=25, Tp=28) == ERR_ARG
    # gamma / beta must match `fold`
    assert call(fold=1, gamma=null) == ERR_ARG and call(fold=1, beta=null) == ERR_ARG
    assert call(fold=1, gamma=null, beta=null) == ERR_ARG
    assert call(fold=0) == ERR_ARG and call(fold=0, gamma=null) == ERR_ARG and call(fold=0, beta=null) == ERR_ARG
    assert call(B=1 << 20, T=1 << 10, Cc=1280) == ERR_ARG          # B T 3C does not fit an int


C_TO_CTYPES = {'const void*': 'c_void_p', 'void*': 'c_void_p', 'const float*': 'c_void_p', 'int': 'c_int'}


def test_ln_qkv_header_and_binding_agree():
    """The declaration of fgdm_op_ln_qkv in include/fgdm.h and its ctypes signature in fgdm_amd/_lib.py: the same argument
    count and, argument by argument, the same kinds (every pointer a c_void_p, every int a c_int), int result; the header
    states the contract next to the other diagnostic entries."""
    hdr = open(os.path.join(ROOT, 'include', 'fgdm.h')).read()
    m = re.search(r'\bint\s+fgdm_op_ln_qkv\s*\(([^)]*)\)\s*;', hdr)
    assert m, 'fgdm_op_ln_qkv is not declared'
    args = [re.sub(r'\s+', ' ', a).strip() for a in m.group(1).split(',')]
    names = [a.split(' ')[-1] for a in args]
    assert names == ['h', 'gamma', 'beta', 'wq', 'wk', 'wv', 'B', 'T', 'C', 'Tp', 'fold', 'qk', 'vt', 'stream'], names
    kinds = [C_TO_CTYPES[a.rsplit(' ', 1)[0]] for a in args]
    res, argtypes = _lib.SIGNATURES['fgdm_op_ln_qkv']
    assert res.__name__ == 'c_int'
    assert [t.__name__ for t in argtypes] == kinds
    doc = re.sub(r'(\s|\*)+', ' ', hdr[hdr.rindex('/*', 0, m.start()):m.start()])       # the comment in front, as one line
    assert 'the product path does not call it' in doc
    for word in ('OUT_F16_T', 'split_n = 2C', 'does NOT clear vt', 'C % 320', 'Tp % 8', 'Tp < T', 'attention.py:180-186'):
        assert word in doc, word


CSRC = os.path.join(ROOT, 'fgdm_amd', 'csrc')


def _csrc_files_with(text):
    return sorted(f for f in os.listdir(CSRC) if f.endswith(('.hip', '.h')) and text in open(os.path.join(CSRC, f)).read())


def test_environment_is_read_through_the_knob_table_only():
    assert _csrc_files_with('getenv(') == ['knobs.h']


def test_knob_table_matches_readme():
    """The names in csrc/knobs.h's table and in the README's table of the native library's switches are the same set."""
    table = re.search(r'#define FGDM_KNOBS\(X\)(.*?)\n\n', open(os.path.join(CSRC, 'knobs.h')).read(), re.S).group(1)
    knobs = set(re.findall(r'"(FGDM_[A-Z0-9_]+)"', table))
    assert len(knobs) >= 29, knobs
    readme = open(os.path.join(ROOT, 'README.md')).read()
    section = readme[readme.index('### Environment switches'):readme.index('Read by the Python side')]
    rows = [ln for ln in section.splitlines() if ln.startswith('| `FGDM_')]
    documented = set(re.findall(r'`(FGDM_[A-Z0-9_]+)', '\n'.join(rows)))
    assert knobs == documented, knobs ^ documented


def test_dynamic_lds_is_opted_in_by_one_helper():
    sites = [(f, open(os.path.join(CSRC, f)).read().count('hipFuncSetAttribute')) for f in _csrc_files_with('hipFuncSetAttribute')]
    assert sites == [('common.h', 1)], sites


def test_engine_needs_gpu_no_fallback(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    with pytest.raises(RuntimeError):
        eng.Engine(gi.SMALL_CFG)
