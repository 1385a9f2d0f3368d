"""TEST INFRASTRUCTURE shared by tools/record_sampler_update_bits.py and tests/test_gpu_sampler_update_bits.py: one list of calls
into the fused sampler updates (fgdm_ddim_step, fgdm_plms_combine, fgdm_axpby, fgdm_mask_blend) and the three loop step kernels
(fgdm_op_ddim_loop_step, fgdm_op_plms_loop_step, fgdm_op_dpmpp_loop_step).  The recorder runs it against one build of the library and
stores inputs and outputs in tests/golden/sampler_update_bits.npz; the test runs it against the build in the tree and compares bit
for bit.  Every output is a poisoned, guarded buffer (tests/guarded.py).  Never imported by the product."""
import ctypes as C

import torch

from guarded import guarded_in, guarded_out

SIZES = (255, 1536)          # odd and less than one block; six full blocks (the 8 x 16 latent of the loop tests)
INPUTS = ('x', 'ec', 'eu', 'noise', 'x0', 'qn', 'mask', 'e1', 'e2', 'e3', 'm1')
# none of them a power of two (tests/test_gpu_ddim_loop.py, tests/test_gpu_multistep_loop.py)
CFG, A_T, A_PREV, SIGMA, S1M, SA2, S1M2 = 7.5, 0.4047, 0.6411, 0.3127, 0.7716, 0.8007, 0.5991
INV_ALPHA, NSA, C1, CM0, CM1 = 1.3971, -0.9757, 0.8312, 0.2714, -0.0931
PROBE, FINISH_FIRST, MULTISTEP = 0, 1, 2
FIRST, SECOND = 1, 2


def make_inputs(n):
    """seeded normal draws and a mask with 0, 1 and soft values (host tensors; the recorder stores them)"""
    g = torch.Generator().manual_seed(n)
    t = {k: torch.randn(n, generator=g) for k in INPUTS if k != 'mask'}
    mask = (torch.rand(n, generator=g) < 0.5).float()
    mask[::7] = 0.3
    t['mask'] = mask
    return t


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def run(lib, host):
    """every call on device copies of `host` (name -> fp32 [n]); returns {case/output: device tensor}"""
    d = {k: guarded_in(v) for k, v in host.items()}
    n = d['x'].numel()
    res = {}

    def call(case, fn, outs, args):
        """fn(*args) with each name of `outs` in args replaced by a guarded output's pointer"""
        bufs = {k: guarded_out((n,), torch.float32) for k in outs}
        rc = fn(*[_p(bufs[a].t) if isinstance(a, str) else a for a in args])
        torch.cuda.synchronize()
        assert rc == 0, (case, rc)
        got = {k: b.check() for k, b in bufs.items()}
        for k in ('xin_a', 'xin_b'):                       # both input halves hold the state: one array is stored
            if k in got and 'x_out' in got:
                assert torch.equal(got.pop(k), got['x_out']), (case, k)
        if 'xin_a' in got and 'xin_b' in got:
            assert torch.equal(got.pop('xin_b'), got['xin_a']), case
        res.update({f'{case}/{k}': v for k, v in got.items()})

    x, ec, eu, noise, x0, qn, mask, e1, e2, e3, m1 = (d[k] for k in INPUTS)
    for cfg_on in (True, False):
        for noisy in (True, False):
            call(f'ddim_step_cfg{int(cfg_on)}_noise{int(noisy)}', lib.fgdm_ddim_step, ('x_prev', 'pred_x0', 'e_out'),
                 (_p(x), _p(ec), _p(eu if cfg_on else None), CFG, A_T, A_PREV, SIGMA if noisy else 0.0, S1M, _p(noise if noisy else None),
                  'x_prev', 'pred_x0', 'e_out', n, None))
    for order in (1, 2, 3):
        call(f'plms_combine_{order}', lib.fgdm_plms_combine, ('out',),
             (_p(ec), _p(e1), _p(e2 if order >= 2 else None), _p(e3 if order >= 3 else None), order, 'out', n, None))
    call('axpby', lib.fgdm_axpby, ('y',), (_p(x0), SA2, _p(qn), S1M2, 'y', n, None))
    call('axpby_b_null', lib.fgdm_axpby, ('y',), (_p(x0), SA2, None, 0.0, 'y', n, None))
    call('mask_blend', lib.fgdm_mask_blend, ('y',), (_p(x0), _p(x), _p(mask), 'y', n, None))

    blend = (_p(mask), _p(x0), _p(qn), SA2, S1M2)
    no_blend = (None, None, None, 0.0, 0.0)
    full = ('x_out', 'xin_a', 'xin_b', 'log_x', 'log_p0')
    call('ddim_loop', lib.fgdm_op_ddim_loop_step, full,
         (_p(x), _p(ec), _p(eu), CFG, A_T, A_PREV, SIGMA, S1M, _p(noise), *blend, *full, n, None))
    call('ddim_loop_plain', lib.fgdm_op_ddim_loop_step, full,
         (_p(x), _p(ec), None, 1.0, A_T, A_PREV, 0.0, S1M, None, *no_blend, *full, n, None))
    call('ddim_loop_no_update', lib.fgdm_op_ddim_loop_step, ('x_out', 'xin_a', 'xin_b'),
         (_p(x), None, None, 0.0, 0.0, 0.0, 0.0, 0.0, None, *blend, 'x_out', 'xin_a', 'xin_b', None, None, n, None))

    def plms(case, e_c, e_u, mode, order, hist, e_out, bl, outs):
        call(case, lib.fgdm_op_plms_loop_step, outs + ((e_out,) if e_out else ()),
             (_p(x), _p(e_c), _p(e_u), CFG, mode, order, *[_p(h) for h in hist], e_out, A_T, A_PREV, S1M, *bl,
              *[k if k in outs else None for k in full], n, None))
    plms('plms_probe', ec, eu, PROBE, 0, (None,) * 3, 'e_out', no_blend, ('xin_a', 'xin_b'))
    plms('plms_finish_first', ec, eu, FINISH_FIRST, 0, (e1, None, None), None, blend, full)
    for order in (1, 2, 3):
        hist = tuple(h if j < order else None for j, h in enumerate((e1, e2, e3)))
        plms(f'plms_multistep_{order}', ec, eu, MULTISTEP, order, hist, 'e_out', blend, full)
    plms('plms_multistep_3_plain', ec, None, MULTISTEP, 3, (e1, e2, e3), 'e_out', no_blend, full)
    plms('plms_no_update', None, None, 0, 0, (None,) * 3, None, blend, ('x_out', 'xin_a', 'xin_b'))

    for kind, name in ((FIRST, 'first'), (SECOND, 'second')):
        for cfg_on in (True, False):
            outs = ('m0_out', 'x_out', 'xin_a', 'xin_b')
            call(f'dpmpp_{name}_cfg{int(cfg_on)}', lib.fgdm_op_dpmpp_loop_step, outs,
                 (_p(x), _p(ec), _p(eu if cfg_on else None), CFG, INV_ALPHA, NSA, _p(m1), kind, C1, CM0, CM1, *outs, n, None))
    return res
