"""Cross-attention maps at the kernel level: fgdm_op_cross_attention_maps (the capturing instantiations of attn_kernel and
attn_cross_kernel plus the head reduction) on the GPU.

Per case (tests/attention_maps_cases.py: d 40 / 64 / 80 / 160, 5 and 8 heads, T 64 / 200 / 256, Tk 77 / 154, B = 3 with every sample
also run alone as B = 1, compact and strided Q | K | O layouts, q_prescaled = 1):
  * O has the bits of fgdm_op_attention_ex on the same operands: the capturing instantiation changes nothing else;
  * every row of maps sums to 1 within 1e-5;
  * maps and O are written inside guarded buffers (tests/guarded.py): nothing outside [B, T, Tk] is touched, nothing inside is left;
  * maps against the float64 mean_heads softmax(Q K^T) of the same fp16 operands, normwise, within the bound measured on the CPU:
    4 x the worst error of a plain fp32 torch evaluation over these cases (fp32 exponentials of fp16 operands on both sides; the
    margin covers the kernel's exp2 and MFMA summation order).  Measured values: profiles/attention_maps_parity_errors.txt;
  * two runs give the same bits (heads are summed in head order), and the B = 3 result equals the three B = 1 results."""
import pytest
import torch

import attention_capture_dispatch as ACD
import attention_maps_cases as MC
from common import report
from guarded import guarded_out
from test_gpu_attention_calls import make_vt, strided_in, vp
from test_gpu_ops import din, _st

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def lib():
    from fgdm_amd import _lib
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return _lib.load()


@pytest.fixture(scope='module')
def bound():
    errs, worst, b = MC.measure_bound()
    return b


def run(lib, case, qs, k, v, maps_entry=True, prescaled=1):
    """one call; returns (O [B T, C] fp16, maps [B, T, Tk] fp32 or None), both checked against their guards"""
    B, Hh, T, Tk, d, layout = case
    Cc, Tkp = Hh * d, (Tk + 63) // 64 * 64
    q2, k2 = qs.reshape(B * T, Cc).half(), k.reshape(B * Tk, Cc).half()
    ldq = ldk = ldo = Cc
    if layout == 'all_different':
        ldq, ldk, ldo = Cc + 8, 2 * Cc + 16, Cc + 4
        qb, kb = strided_in(q2, ldq), strided_in(k2, ldk)
    else:
        qb, kb = din(q2), din(k2)
    vtd = din(make_vt(v, B, Tk, Cc, Tkp))
    out = guarded_out((B * T, ldo), torch.half)
    head = (vp(qb.data_ptr()), ldq, vp(kb.data_ptr()), ldk, vp(vtd.data_ptr()), Tkp, vp(out.data_ptr()), ldo)
    maps = None
    if maps_entry:
        maps = guarded_out((B, T, Tk), torch.float32)
        rc = lib.fgdm_op_cross_attention_maps(*head, vp(maps.data_ptr()), B, Hh, T, Tk, d, prescaled, _st())
    else:
        rc = lib.fgdm_op_attention_ex(*head, B, Hh, T, Tk, d, prescaled, _st())
    assert rc == 0, (MC.case_id(case), rc)
    torch.cuda.synchronize()
    region = (slice(None), slice(0, Cc))
    out.check(region)
    if ldo > Cc:
        out.assert_untouched((slice(None), slice(Cc, ldo)))
    if maps is not None:
        assert lib.fgdm_debug_last_attention_kernel() == ACD.expected_capture_kernel(T, Tk, d), MC.case_id(case)
        maps.check()
    return out.t[region].clone(), None if maps is None else maps.t.clone()


@pytest.mark.parametrize('case', MC.CASES, ids=MC.case_id)
def test_maps(lib, bound, case):
    B, Hh, T, Tk, d, layout = case
    qs, k, v = MC.inputs(case)
    o, maps = run(lib, case, qs, k, v)
    o_plain, _ = run(lib, case, qs, k, v, maps_entry=False)
    assert torch.equal(o, o_plain), 'O of the capturing instantiation differs from fgdm_op_attention_ex'
    sums = maps.sum(-1)
    print(f'{MC.case_id(case)}: row sums in [{float(sums.min()):.7f}, {float(sums.max()):.7f}]')
    assert float((sums - 1).abs().max()) < 1e-5
    ref = MC.maps_reference(qs, k, B, Hh, d)
    err = report(f'attention maps {MC.case_id(case)}: kernel vs float64', MC.relerr(maps.cpu(), ref), bound)
    assert err < bound, MC.case_id(case)
    # determinism, and independence of the batch: each sample alone gives the rows it has in the batch
    o2, maps2 = run(lib, case, qs, k, v)
    assert torch.equal(maps2, maps) and torch.equal(o2, o)
    for b in range(B):
        one = (1,) + case[1:]
        ob, mb = run(lib, one, qs[b:b + 1], k[b:b + 1], v[b:b + 1])
        assert torch.equal(mb[0], maps[b]) and torch.equal(ob, o[b * T:(b + 1) * T]), f'sample {b} alone differs from its rows in the batch'


@pytest.mark.parametrize('case', [c for c in MC.CASES if c[1] == 5 and c[2] == 200 and c[5] == 'compact'], ids=MC.case_id)
def test_unscaled_q_keeps_o_and_row_sums(lib, case):
    """q_prescaled = 0: the kernels scale Q themselves (d = 40: rounded to fp16 once more, so no float64 bar here)"""
    qs, k, v = MC.inputs(case)
    o, maps = run(lib, case, qs, k, v, prescaled=0)
    o_plain, _ = run(lib, case, qs, k, v, maps_entry=False, prescaled=0)
    assert torch.equal(o, o_plain)
    assert float((maps.sum(-1) - 1).abs().max()) < 1e-5


def test_refusals(lib):
    """before any launch: more keys than the capturing kernels take, and shapes the dispatch gives to the self-attention kernels"""
    case = (1, 2, 256, 77, 40, 'compact')
    qs, k, v = MC.inputs(case)
    B, Hh, T, Tk, d, _ = case
    Cc = Hh * d
    q, kk, vt = din(qs.reshape(T, Cc).half()), din(torch.zeros(320, Cc).half()), din(torch.zeros(Cc, 320).half())
    out, maps = guarded_out((T, Cc), torch.half), guarded_out((1, T, 320), torch.float32)
    for tk in (257, 320, 128, 256):
        assert ACD.expected_capture_kernel(T, tk, d) is None
        rc = lib.fgdm_op_cross_attention_maps(vp(q.data_ptr()), Cc, vp(kk.data_ptr()), Cc, vp(vt.data_ptr()), 320, vp(out.data_ptr()), Cc,
                                              vp(maps.data_ptr()), 1, Hh, T, tk, d, 1, _st())
        assert rc == -1, tk
    torch.cuda.synchronize()
    out.check_guards(), maps.check_guards()
    out.assert_untouched((slice(None), slice(None))), maps.assert_untouched((slice(None),) * 3)
