"""Upsample convs as four 2x2 phase GEMMs (IG_CONV2_PHASE; DESIGN.md, "Upsample convs as four 2x2 phase GEMMs"): nearest-2x + conv3x3 through fgdm_op_conv2d, which takes the
engine's dispatch (igemm_up_phase), with FGDM_IGEMM_UP_PHASE on (the phase form) and off (the 3x3 walk over the virtual upsampled
image).  The launcher knobs are read once per process, so each knob setting runs all cases in one fresh child process (two children for
the whole file); the float64 CPU reference is computed once per case here and shared by every test.

The phase form serves one source of at least 8 x 8 pixels with C % 64 == 0 and N % 320 == 0 (the UNets' Upsample layers).  Case (2, 8, 8, 128, 64) has N = 64
and stays on the 3x3 walk under either knob setting (the rule is geometry only): it checks that the rule leaves such a layer
alone (two images inside one tile on the phase path: the 8x8 C640 N640 case).  The C++ packer's output is not readable through the lib ABI; its bits are covered by the
op-level parity here and its arithmetic by the numpy transcription in test_upsample_phase_pack.py.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_ops import LOCAL_TOL, TOL, close, h16, rnd, to_rows

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

#        B, H, W, C, N, act
CASES = [(2, 8, 8, 128, 64, 0),
         (3, 8, 16, 64, 320, 0),
         (2, 4, 4, 640, 640, 0),
         (2, 8, 8, 640, 1280, 1),
         # sources below 8 x 8 stay on the 3x3 walk as well (igemm_up_phase), so the 4x4 case above runs it under both settings; these two
         # put its properties on the phase path: tile rows spanning several source rows and both images with several K chunks per tap,
         # and an odd batch whose last image ends inside a tile (M = 320 of 384 rows)
         (2, 8, 8, 640, 640, 0),
         (5, 8, 8, 128, 320, 0)]
IDS = ['B2 8x8 C128 N64', 'B3 8x16 C64 N320', 'B2 4x4 C640 N640', 'B2 8x8 C640 N1280 silu', 'B2 8x8 C640 N640', 'B5 8x8 C128 N320']
ON_PHASE = [1, 3, 4, 5]        # cases the phase form serves when the knob is on


def _inputs(case):
    B, H, W, Cc, N, act = case
    x = h16(rnd((B, Cc, H, W), 11))                             # fp16-rounded input
    w = rnd((N, Cc, 3, 3), 12, 1.0 / np.sqrt(Cc * 9))           # fp32 weights (NOT fp16-representable: the phase sums round once)
    bias = rnd((N,), 13, 0.1)
    return x, w, bias


_refs = {}


def reference(case):
    """float64 on the CPU: F.interpolate(nearest, 2x) then conv2d.  [B, N, 2H, 2W]; computed once, never modified."""
    if case not in _refs:
        x, w, bias = _inputs(case)
        r = F.conv2d(F.interpolate(x.double(), scale_factor=2, mode='nearest'), w.double(), bias.double(), padding=1)
        if case[5] == 1:
            r = F.silu(r)
        _refs[case] = r
    return _refs[case]


CHILD = r'''
import ctypes as C, json, os, sys
sys.path.insert(0, os.path.join({root!r}, 'tests')); sys.path.insert(0, {root!r})
import torch
from guarded import guarded_in, guarded_out
from fgdm_amd import _lib
import test_gpu_upsample_phase as T
lib = _lib.load()
res = {{}}
p = lambda t: C.c_void_p(t.data_ptr())
for ci, case in enumerate(T.CASES):
    B, H, W, Cc, N, act = case
    x, w, bias = T._inputs(case)
    wd, bd = w.cuda(), bias.cuda()
    for nb in (1, B):        # the first nb samples of the case's batch
        xd = guarded_in(x[:nb].permute(0, 2, 3, 1).half().contiguous())
        out = guarded_out((nb * 4 * H * W, N), torch.half)
        rc = lib.fgdm_op_conv2d(p(xd), Cc, C.c_void_p(0), 0, p(wd), p(bd), C.c_void_p(0), C.c_void_p(0), nb, H, W, N, 3, 1, 1, act,
                                C.c_float(1.0), p(out.t), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, (case, rc)
        torch.cuda.synchronize()
        res[(ci, nb)] = out.check().cpu().clone()     # guards intact, no poison left anywhere in the output, finite
torch.save(res, sys.argv[1])
'''

_runs = {}


def run(case, knob, tmp_path_factory):
    '''every case through the op entry in ONE child process per knob setting (FGDM_IGEMM_UP_PHASE=knob), at B = 1 and at the case's
    batch -> {batch: [batch * 2H * 2W, N] fp16} of `case`'''
    if knob not in _runs:
        outp = str(tmp_path_factory.mktemp('upphase') / 'out.pt')
        env = dict(os.environ, FGDM_IGEMM_UP_PHASE=str(knob))
        r = subprocess.run([sys.executable, '-c', CHILD.format(root=ROOT), outp], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        _runs[knob] = torch.load(outp)
    ci = CASES.index(case)
    return {str(nb): _runs[knob][(ci, nb)] for nb in (1, case[0])}


def _errs(got, ref_rows):
    d = (got.double() - ref_rows).abs()
    return float(d.max()), float(d.mean())


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_parity_phase_and_3x3_against_float64(case, tmp_path_factory):
    B, H, W, Cc, N, act = case
    ref_rows = to_rows(reference(case))
    lines = []
    for knob in (1, 0):
        got = run(case, knob, tmp_path_factory)[str(B)]
        mx, mean = _errs(got, ref_rows)
        e = float((got.double() - ref_rows).norm() / ref_rows.norm())
        print(f'upsample {case} FGDM_IGEMM_UP_PHASE={knob}: max {mx:.3e} mean {mean:.3e} normwise {e:.3e}')
        lines.append(f'{IDS[CASES.index(case)]:26s} UP_PHASE={knob}  max_abs {mx:.3e}  mean_abs {mean:.3e}  normwise {e:.3e}')
        close(f'upsample phase={knob} {case}', got.cuda(), ref_rows, TOL, LOCAL_TOL)
    path = os.environ.get('FGDM_UP_PHASE_PARITY_LOG')      # profiles/upsample_phase_parity_errors.txt is a copy of one such run
    if path:
        with open(path, 'a') as f:
            f.write('\n'.join(lines) + '\n')


@pytest.mark.parametrize('case', [CASES[i] for i in ON_PHASE], ids=[IDS[i] for i in ON_PHASE])
def test_every_element_written_once_and_borders(case, tmp_path_factory):
    """No poison left and guards intact (out.check() in the child); then the four border rows / columns of every image on their
    own, so a wrong displacement at a = 0 / b = 0 (or at the far edge) cannot average away in the whole-tensor norm.  Bound: the
    conv tolerance TOL on each line's normwise error (a line has >= 8 * N >= 2560 elements: fp16 storage and the once-rounded
    weights give ~3e-4 there as everywhere; a wrong or missing tap changes a line by tens of percent)."""
    B, H, W, Cc, N, act = case
    got = run(case, 1, tmp_path_factory)[str(B)].double().view(B, 2 * H, 2 * W, N)
    ref = reference(case).permute(0, 2, 3, 1)
    for b in range(B):
        for name, sl in (('top', (b, 0)), ('bottom', (b, 2 * H - 1)), ('left', (b, slice(None), 0)), ('right', (b, slice(None), 2 * W - 1))):
            g, r = got[sl], ref[sl]
            e = float((g - r).norm() / r.norm())
            assert e < TOL, (case, b, name, e)
        # ... and the second / second-to-last lines: the first ones whose taps all lie inside the image
        for name, sl in (('row 1', (b, 1)), ('row -2', (b, 2 * H - 2)), ('col 1', (b, slice(None), 1)), ('col -2', (b, slice(None), 2 * W - 2))):
            g, r = got[sl], ref[sl]
            assert float((g - r).norm() / r.norm()) < TOL, (case, b, name)


@pytest.mark.parametrize('case', [CASES[i] for i in ON_PHASE], ids=[IDS[i] for i in ON_PHASE])
def test_sample_bits_do_not_depend_on_the_batch(case, tmp_path_factory):
    B, H, W, Cc, N, act = case
    r = run(case, 1, tmp_path_factory)
    one, many = r['1'], r[str(B)]
    assert torch.equal(one.view(torch.int16), many[:4 * H * W].view(torch.int16))
