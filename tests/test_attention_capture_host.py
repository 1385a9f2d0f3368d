"""Cross-attention capture without a device: the header, the ctypes mirror and the _SIZE_V1 define agree; the entries refuse NULL
and bad arguments before they touch a device; block names resolve against the walk order of csrc/model.h."""
import ctypes as C
import os
import re

import pytest

import golden_inputs as gi
from fgdm_amd import _lib
from fgdm_amd import engine as E

HDR = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'fgdm.h')


def _lib_loaded():
    if not os.path.exists(_lib.LIB_PATH):
        from fgdm_amd import build
        build.build(verbose=False)
    return _lib.load()


def test_header_mirror_and_size_define_agree():
    hdr = open(HDR).read()
    size_v1 = int(re.search(r'#define FGDM_ATTENTION_CAPTURE_SIZE_V1 (\d+)', hdr).group(1))
    body = re.search(r'typedef struct fgdm_attention_capture \{(.*?)\} fgdm_attention_capture;', hdr, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names = []
    for decl in body.split(';'):
        decl = decl.strip()
        if decl:
            first, *rest = decl.split(',')
            names += [first.split()[-1].lstrip('*')] + [r.strip() for r in rest]
    assert names == [f[0] for f in _lib.FgdmAttentionCapture._fields_]
    assert C.sizeof(_lib.FgdmAttentionCapture) == size_v1 == 48
    assert _lib.FgdmAttentionCapture.block_mask.offset == 16 and _lib.FgdmAttentionCapture.reserved0.offset == 44
    assert int(re.search(r'#define FGDM_ATTENTION_CAPTURE_MAX_KEYS (\d+)', hdr).group(1)) == _lib.ATTENTION_CAPTURE_MAX_KEYS
    for name, val in (('ROWS_ALL', 0), ('ROWS_COND', 1), ('ROWS_UNCOND', 2), ('SUM', 0), ('LAST', 1)):
        assert int(re.search(rf'#define FGDM_CAPTURE_{name} (\d+)', hdr).group(1)) == val
    assert _lib.CAPTURE_ROWS == {'all': 0, 'cond': 1, 'uncond': 2} and _lib.CAPTURE_MODES == {'sum': 0, 'last': 1}
    for fn in ('fgdm_attention_capture_set', 'fgdm_attention_capture_reset', 'fgdm_attention_capture_info',
               'fgdm_attention_capture_block_size', 'fgdm_attention_capture_read', 'fgdm_op_cross_attention_maps'):
        assert fn in _lib.SIGNATURES and re.search(rf'\bint {fn}\(', hdr), fn
    doc = re.sub(r'(\s|\*)+', ' ', hdr[hdr.index('Cross-attention maps: what'):hdr.index('typedef struct fgdm_attention_capture')])
    for word in ('attention.py:177-216', 'IN HEAD ORDER', 'NOT captured: the ControlNets', 'FGDM_ATTENTION_CAPTURE_MAX_KEYS',
                 'FGDM_ERR_ARG before any launch', 'DIVIDED BY NOTHING'):
        assert word in doc, word


def test_entries_refuse_null_and_bad_arguments_without_a_device():
    lib = _lib_loaded()
    plan = _lib.FgdmAttentionCapture()
    plan.struct_size = C.sizeof(plan)
    plan.block_mask = 1
    assert lib.fgdm_attention_capture_set(None, C.byref(plan)) == -1 and lib.fgdm_attention_capture_set(None, None) == -1
    assert lib.fgdm_attention_capture_reset(None, None) == -1
    shape, n, h = (C.c_int64 * 3)(), C.c_int32(), C.c_int32()
    assert lib.fgdm_attention_capture_info(None, 0, shape, C.byref(n)) == -1
    assert lib.fgdm_attention_capture_block_size(None, 0, C.byref(h), C.byref(h)) == -1
    assert lib.fgdm_attention_capture_read(None, 0, C.c_void_p(1 << 20), None) == -1
    q, null = C.c_void_p(1 << 20), None

    def maps(qp=q, kp=q, vt=q, o=q, m=q, B=1, heads=2, T=128, Tk=77, d=40):
        return lib.fgdm_op_cross_attention_maps(qp, 80, kp, 80, vt, 128, o, 80, m, B, heads, T, Tk, d, 1, None)
    for kw in (dict(qp=null), dict(kp=null), dict(vt=null), dict(o=null), dict(m=null), dict(B=0), dict(heads=0), dict(T=0), dict(Tk=0),
               dict(Tk=_lib.ATTENTION_CAPTURE_MAX_KEYS + 1), dict(d=48)):
        assert maps(**kw) == -1, kw


class StubEngine(E.Engine):
    """the Python side of an engine without the native one: what capture_attention resolves names against"""

    def __init__(self, cfg):
        self.config = E.make_config(cfg)


def test_block_names_resolve_against_the_walk_order():
    sd = StubEngine(gi.SD_CFG)
    table = E.attention_blocks(sd.config)
    # model.h: input blocks (two per level with attention, levels at ds 1, 2, 4), the middle block at ds 8, output blocks (three per level)
    assert table == [('down', 1)] * 2 + [('down', 2)] * 2 + [('down', 4)] * 2 + [('mid', 8)] + [('up', 4)] * 3 + [('up', 2)] * 3 + [('up', 1)] * 3
    cap = sd.capture_attention
    assert cap().blocks == list(range(16))
    assert cap('down').blocks == [0, 1, 2, 3, 4, 5] and cap('mid').blocks == [6] and cap('up').blocks == list(range(7, 16))
    assert cap(blocks='16', latent=64).blocks == [4, 5, 7, 8, 9]          # the five 16 x 16 blocks of a 64 x 64 latent: ds 4
    assert cap(blocks=[('up', 32)], latent=64).blocks == [10, 11, 12] and cap(blocks=('down', 64), latent=64).blocks == [0, 1]
    assert cap(blocks=[3, 'mid', 3]).blocks == [3, 6]
    small = StubEngine(gi.SMALL_CFG)
    assert E.attention_blocks(small.config) == [('down', 1), ('down', 2), ('mid', 2), ('up', 2), ('up', 2), ('up', 1), ('up', 1)]
    plan = small.capture_attention(blocks=['mid', 0], tokens=[1, 5], rows='uncond', mode='last').plan
    assert (plan.block_mask, plan.n_tokens, plan.rows, plan.mode, plan.struct_size) == (0b101, 2, 2, 1, 48)
    assert [plan.tokens[i] for i in range(2)] == [1, 5]
    for bad in (dict(blocks='sideways'), dict(blocks=16), dict(blocks='16'), dict(blocks='7', latent=64), dict(rows='both'), dict(mode='mean')):
        with pytest.raises(ValueError):
            sd.capture_attention(**bad)


def test_latent_diffusion_takes_a_side_as_an_int():
    from fgdm_amd import models

    class StubLDM(models.LatentDiffusion):
        def __init__(self):
            self.engine, self.image_size = StubEngine(gi.SD_CFG), 64
    m = StubLDM()
    assert m.capture_attention(16).blocks == [4, 5, 7, 8, 9] and m.capture_attention(['mid', 64]).blocks == [0, 1, 6, 13, 14, 15]
    assert m.capture_attention(8, latent=32).blocks == [4, 5, 7, 8, 9]
