"""TEST INFRASTRUCTURE shared by tools/make_dpm_solver_goldens.py (which runs the REFERENCE's DPM_Solver.sample over these cases and
records tests/golden/dpm_solver.npz), tests/test_dpm_solver_host.py (CPU) and tests/test_gpu_dpm_solver_loop.py (GPU): the list of
solver configurations, and torch / numpy stand-ins of the one kernel behind the per-step route (fgdm_op_dpm_program_step).  Never
imported by the product."""
import numpy as np
import torch

# name -> (predict_x0, guidance scale, DPM_Solver.sample keywords)
CASES = {}


def _case(name, px0, scale=7.5, **kw):
    CASES[name + ('_x0' if px0 else '_eps') + f'_s{scale}'] = (px0, scale, kw)


for _px0 in (True, False):
    for _order in (1, 2, 3):
        for _S in (10, 20):                                     # S = 10: lower_order_final is active
            _case(f'multistep_o{_order}_S{_S}', _px0, method='multistep', order=_order, steps=_S)
    for _order in (2, 3):
        for _S in (10, 11):                                     # S = 11: an uneven order split
            _case(f'singlestep_o{_order}_S{_S}', _px0, method='singlestep', order=_order, steps=_S)
    _case('multistep_o3_S10_nolof', _px0, method='multistep', order=3, steps=10, lower_order_final=False)
    _case('fixed_o3_S12', _px0, method='singlestep_fixed', order=3, steps=12)
    for _skip in ('logSNR', 'time_quadratic'):
        _case(f'multistep_o2_S10_{_skip}', _px0, method='multistep', order=2, steps=10, skip_type=_skip)
        _case(f'singlestep_o3_S10_{_skip}', _px0, method='singlestep', order=3, steps=10, skip_type=_skip)
    _case('multistep_o2_S10_taylor', _px0, method='multistep', order=2, steps=10, solver_type='taylor')
    _case('singlestep_o2_S10_taylor', _px0, method='singlestep', order=2, steps=10, solver_type='taylor')
    _case('singlestep_o3_S9_taylor', _px0, method='singlestep', order=3, steps=9, solver_type='taylor')
    _case('multistep_o2_S10_dz', _px0, method='multistep', order=2, steps=10, denoise_to_zero=True)
    _case('singlestep_o3_S10_dz', _px0, method='singlestep', order=3, steps=10, denoise_to_zero=True)
    _case('multistep_o3_S20_tend', _px0, method='multistep', order=3, steps=20, t_end=0.01)
    _case('singlestep_o3_S10_tstart_tend', _px0, method='singlestep', order=3, steps=10, t_start=0.8, t_end=0.02)
    _case('multistep_o2_S10', _px0, scale=1.0, method='multistep', order=2, steps=10)
    _case('singlestep_o3_S10', _px0, scale=1.0, method='singlestep', order=3, steps=10)


def fma_f32(a, b, c):
    """float32 fma(a, b, c) elementwise, exactly: a * b is exact in float64 (24 + 24 bits); the float64 sum with c is rounded to ODD
    (where it is inexact, of the two float64 neighbours of the exact sum the one with an odd last bit is taken; two-sum gives the
    side), and a round-to-odd value of 53 bits rounds to 24 bits like the exact sum.  Finite, normal values only."""
    a, b, c = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in np.broadcast_arrays(a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)                 # exact: p + c == s + err
    even = (s.view(np.int64) & 1) == 0
    towards = np.where(err > 0, np.inf, -np.inf)
    s = np.where((err != 0) & even, np.nextafter(s, towards), s)
    return s.astype(np.float32)


def emulate_step(x_eval, ec, eu, cfg, conv_x, conv_e, base, hist, planes, coefs):
    """k_dpm_program_step on numpy float32 arrays with the kernel's explicit roundings -> (m, acc):
    e = fma(cfg, ec - eu, eu);  m = e, or fma(conv_x, x_eval, conv_e * e);  acc = coef_0 p_0, then fma(coef_j, p_j, acc) in order"""
    f = np.float32
    e = ec if eu is None else fma_f32(f(cfg), (ec - eu).astype(f), eu)
    m = e if conv_x == 0 else fma_f32(f(conv_x), x_eval, (f(conv_e) * e).astype(f))
    src = [base, hist[0], hist[1], hist[2], m]
    acc = (f(coefs[0]) * src[planes[0]]).astype(f)
    for c, p in zip(coefs[1:], planes[1:]):
        acc = fma_f32(f(c), src[p], acc)
    return m, acc


class Stubs:
    """torch-CPU stand-ins for what fgdm_amd.dpm_solver calls through `_k` (same formulas, torch's own rounding)"""

    @staticmethod
    def cfg_combine(e_c, e_u, s):
        return e_u + s * (e_c - e_u)

    @staticmethod
    def dpm_program_step(x_eval, e_cond, e_uncond, cfg_scale, conv_x, conv_e, base, hist, slot, planes, coefs):
        e = e_cond if e_uncond is None else e_uncond + cfg_scale * (e_cond - e_uncond)
        m = e if conv_x == 0 else conv_x * x_eval + conv_e * e
        src = [base, hist[0], hist[1], hist[2], m]
        vals = [src[p].clone() for p in planes]                 # every plane is read before the slot is written
        if slot >= 0:
            hist[slot].copy_(m)
        acc = coefs[0] * vals[0]
        for c, v in zip(coefs[1:], vals[1:]):
            acc = acc + c * v
        return acc


def run_device_loop(step, net, x_T, cond, uncond, cfg_scale, prog):
    """fgdm_sample_dpm_solver as its header comment describes it: per record the network on the evaluation input at t_float[k],
    then one launch (`step`: the signature of fgdm_amd.engine.dpm_program_step); the result becomes the next evaluation input and,
    behind a DEST_STATE record, the state"""
    cfg_on = uncond is not None and cfg_scale != 1.0
    x, xin = x_T, x_T
    hist = [torch.empty_like(x_T) for _ in range(3)]
    for k in range(len(prog['t_float'])):
        t = torch.full((x.shape[0],), prog['t_float'][k], dtype=torch.float32, device=x.device)
        if cfg_on:
            e_u, e_c = net(torch.cat([xin] * 2), torch.cat([t] * 2), torch.cat([uncond, cond])).chunk(2)
            e_c, e_u = e_c.contiguous(), e_u.contiguous()
        else:
            e_c, e_u = net(xin, t, cond), None
        n = prog['nterms'][k]
        xin = step(xin, e_c, e_u, cfg_scale, prog['conv_x'][k], prog['conv_e'][k], x, hist, prog['slot'][k], prog['plane'][k][:n],
                   prog['coef'][k][:n])
        if prog['dest'][k] == 1:
            x = xin
    return x
