"""TEST INFRASTRUCTURE shared by tools/record_ancestral_update_bits.py and tests/test_gpu_ancestral_update_bits.py: one list of calls
into fgdm_ancestral_step (k_ancestral), which tests/sampler_update_cases.py does not cover.  The recorder runs it against one build
of the library and stores inputs and outputs in tests/golden/ancestral_update_bits.npz; the test runs it against the build in the
tree and compares bit for bit.  Every output is a poisoned, guarded buffer (tests/guarded.py).  Never imported by the product."""
import ctypes as C

import torch

from guarded import guarded_in, guarded_out

SIZES = (255, 1536)          # odd and less than one block; six full blocks (the sizes of tests/sampler_update_cases.py)
INPUTS = ('x', 'eps', 'noise', 'x_small', 'eps_wide')
# (sqrt_recip_ac, sqrt_recipm1_ac, coef1, coef2, std) as the linear schedule holds them near t = 500, t = 999 and t = 1; none of
# them a power of two
COEFS = {
    't500': (1.5719, 1.2128, 0.0127, 0.9871, 0.0631),
    't999': (14.6488, 14.6146, 0.0049, 0.9940, 0.1091),
    't1': (1.0009, 0.0413, 0.4988, 0.5008, 0.0206),
}
SIGNATURE = (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p,
                       C.c_int64, C.c_void_p])


def make_inputs(n):
    """seeded draws (host tensors; the recorder stores them): unit normals, and a pair whose dynamic range -- x near 0 against
    |eps| from 1e-2 up to 1e4 -- makes a product fused into the wrong sum, or not fused, visible"""
    g = torch.Generator().manual_seed(7000 + n)
    t = {k: torch.randn(n, generator=g) for k in ('x', 'eps', 'noise')}
    t['x_small'] = torch.randn(n, generator=g) * 1e-3
    t['eps_wide'] = torch.randn(n, generator=g) * 10.0 ** (-2.0 + 6.0 * torch.rand(n, generator=g))
    return t


def bind(lib):
    """fgdm_ancestral_step of a ctypes library handle, with its signature (a build of an older commit may lack the symbols
    fgdm_amd._lib.load() insists on, so the recorder binds this one alone)"""
    fn = lib.fgdm_ancestral_step
    fn.restype, fn.argtypes = SIGNATURE
    return fn


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def run(fn, host):
    """every call on device copies of `host` (name -> fp32 [n]); returns {case: device tensor}"""
    d = {k: guarded_in(v) for k, v in host.items()}
    n = d['x'].numel()
    res = {}
    for pair, (x, eps) in (('unit', (d['x'], d['eps'])), ('wide', (d['x_small'], d['eps_wide']))):
        for name, (cr, crm1, c1, c2, std) in COEFS.items():
            # noise on; noise NULL (the t == 0 step); std == 0 with the noise handed over all the same
            for case, s, nz in (('noise', std, d['noise']), ('no_noise', std, None), ('std0', 0.0, d['noise'])):
                out = guarded_out((n,), torch.float32)
                rc = fn(_p(x), _p(eps), cr, crm1, c1, c2, s, _p(nz), _p(out.t), n, None)
                torch.cuda.synchronize()
                assert rc == 0, (pair, name, case, rc)
                res[f'{pair}_{name}_{case}'] = out.check()
    return res
