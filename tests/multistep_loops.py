"""TEST INFRASTRUCTURE shared by tests/test_multistep_loop_host.py (CPU) and tests/test_gpu_multistep_loop.py (GPU): the device PLMS
and DPM-Solver++ loops restated in Python exactly as include/fgdm.h documents them (fgdm_sample_plms: probe, finish-first,
multistep with three rotating history planes; fgdm_sample_dpmpp: evaluate, then update), over a `step` function that stands for
ONE launch of the step kernel:

  plms_chain(k) / dpmpp_chain(k)   the chain of existing kernels that one launch fuses, k = kernel_stubs (CPU) or
                                   fgdm_amd.engine (the HIP kernels): cfg_combine -> plms_combine / axpby -> ddim_step ->
                                   axpby + mask_blend, and cfg_combine -> axpby -> axpby (-> axpby)
  (the GPU tests pass a step that calls fgdm_op_plms_loop_step / fgdm_op_dpmpp_loop_step instead)

and a stand-in engine (LoopEngine) whose sample_plms / sample_dpmpp run these loops on a closed-form network, so that a sampler's
device route can be followed to its result without the library's networks.  Never imported by the product."""
import torch

PROBE, FINISH_FIRST, MULTISTEP = 0, 1, 2
FIRST, SECOND = 1, 2


def plms_chain(k):
    """step(x, ec, eu, cfg, mode, order, (e1, e2, e3), a_t, a_prev, s1m, blend) -> (e_t, x, xin, log_x, log_pred_x0);
    blend: None or (mask, x0, q_noise, sqrt_ac_next, sqrt_one_minus_ac_next).  The probe returns x = None (the state is untouched)."""
    def step(x, ec, eu, cfg, mode, order, hist, a_t, a_prev, s1m, blend):
        e = xp = p0 = None
        if ec is None:
            xp = x
        else:
            e = ec if eu is None else k.cfg_combine(ec, eu, cfg)
            if mode == PROBE:
                ep = e
            elif mode == FINISH_FIRST:
                ep = k.axpby(hist[0], 0.5, e, 0.5)
            else:
                ep = k.plms_combine(e, list(reversed(hist[:order])))          # old_eps[-1] is e1
            xp, p0 = k.ddim_step(x, ep, None, 1.0, a_t, a_prev, 0.0, s1m, None)
            if mode == PROBE:
                return e, None, xp, None, None
        xn = xp
        if blend is not None:
            mask, x0, qn, sa, s1m_next = blend
            xn = k.mask_blend(k.axpby(x0, sa, qn, s1m_next), xp, mask)
        return e, xn, xn, xp, p0
    return step


def dpmpp_chain(k):
    """step(x, ec, eu, cfg, inv_alpha, neg_sigma_over_alpha, m1, kind, c1, cm0, cm1) -> (m0, x)"""
    def step(x, ec, eu, cfg, inv_alpha, nsa, m1, kind, c1, cm0, cm1):
        e = ec if eu is None else k.cfg_combine(ec, eu, cfg)
        m0 = k.axpby(x, inv_alpha, e, nsa)
        y = k.axpby(x, c1, m0, cm0)
        return m0, (y if kind == FIRST else k.axpby(y, 1.0, m1, cm1))
    return step


def _evaluator(net, cond, uncond, cfg_on):
    """the network on cat([x] * 2) / cat([uncond, cond]) (or on x alone) -> (e_cond, e_uncond)"""
    def evaluate(xin, t):
        if not cfg_on:
            return net(xin, t, cond), None
        e_u, e_c = net(torch.cat([xin] * 2), torch.cat([t] * 2), torch.cat([uncond, cond])).chunk(2)
        return e_c.contiguous(), e_u.contiguous()
    return evaluate


def run_plms_loop(step, net, x_T, cond, uncond, cfg_scale, timesteps, alphas, alphas_prev, s1m, mask=None, x0=None, q_noise=None,
                  sqrt_alphas_cumprod_t=None, sqrt_one_minus_alphas_cumprod_t=None, log_steps=(), trace=None):
    """fgdm_sample_plms as its header comment describes it.  trace: a list that receives (mode, order) of every launch."""
    S = len(timesteps)
    evaluate = _evaluator(net, cond, uncond, uncond is not None and cfg_scale != 1.0)
    at = lambda k: torch.full((x_T.shape[0],), int(timesteps[k]), dtype=torch.long, device=x_T.device)
    blend = lambda i: None if mask is None else (mask, x0, q_noise[i], float(sqrt_alphas_cumprod_t[S - 1 - i]),
                                                 float(sqrt_one_minus_alphas_cumprod_t[S - 1 - i]))
    note = (lambda *a: None) if trace is None else (lambda *a: trace.append(a))
    x = x_T
    _, xn, xin, _, _ = step(x, None, None, 0.0, 0, 0, (None,) * 3, 0.0, 0.0, 0.0, blend(0))      # in front of the first step
    if mask is not None:
        x = xn
    planes, x_inter, pred_x0 = [None] * 3, [], []
    for i in range(S):
        k = S - 1 - i
        ec, eu = evaluate(xin, at(k))
        coef = (float(alphas[k]), float(alphas_prev[k]), float(s1m[k]))
        nxt = blend(i + 1) if i + 1 < S else None
        if i == 0:
            note(PROBE, 0)
            planes[0], _, xin, _, _ = step(x, ec, eu, cfg_scale, PROBE, 0, (None,) * 3, *coef, None)
            ec, eu = evaluate(xin, at(max(S - 2, 0)))
            note(FINISH_FIRST, 0)
            _, x, xin, lx, lp = step(x, ec, eu, cfg_scale, FINISH_FIRST, 0, (planes[0], None, None), *coef, nxt)
        else:
            order = min(i, 3)
            hist = tuple(planes[(i - j) % 3] if j <= order else None for j in (1, 2, 3))
            note(MULTISTEP, order)
            planes[i % 3], x, xin, lx, lp = step(x, ec, eu, cfg_scale, MULTISTEP, order, hist, *coef, nxt)
        if i in log_steps:
            x_inter.append(lx)
            pred_x0.append(lp)
    return x, (torch.stack(x_inter) if x_inter else None), (torch.stack(pred_x0) if pred_x0 else None)


def run_dpmpp_loop(step, net, x_T, cond, uncond, cfg_scale, tab):
    """fgdm_sample_dpmpp as its header comment describes it: per evaluation k the network at t_float[k], then one launch"""
    evaluate = _evaluator(net, cond, uncond, uncond is not None and cfg_scale != 1.0)
    x, m1 = x_T, None
    for k in range(len(tab['t_float'])):
        t = torch.full((x.shape[0],), tab['t_float'][k], dtype=torch.float32, device=x.device)
        ec, eu = evaluate(x, t)
        m1, x = step(x, ec, eu, cfg_scale, tab['inv_alpha'][k], tab['neg_sigma_over_alpha'][k], m1, tab['update_kind'][k],
                     tab['c1'][k], tab['cm0'][k], tab['cm1'][k])
    return x


class LoopEngine:
    """An engine without networks: records what the samplers hand to sample_plms / sample_dpmpp and runs the documented loops
    over `net` (x, t, context) -> eps with the given step functions."""
    has_vae, has_vae_encoder, has_clip = False, False, False

    def __init__(self, net, plms_step, dpmpp_step, device='cpu'):
        self.net, self.plms_step, self.dpmpp_step = net, plms_step, dpmpp_step
        self.device = torch.device(device)
        self.plms, self.dpmpp, self.trace = [], [], []

    def sample_plms(self, x_T, cond, uncond, cfg_scale, timesteps, alphas, alphas_prev, sqrt_one_minus_alphas, control_scales=None,
                    flags=0, **kw):
        self.plms.append(dict(kw, x_T=x_T, cond=cond, uncond=uncond, cfg_scale=cfg_scale, timesteps=list(timesteps), alphas=alphas,
                              alphas_prev=alphas_prev, sqrt_one_minus_alphas=sqrt_one_minus_alphas, control_scales=control_scales,
                              flags=flags))
        return run_plms_loop(self.plms_step, self.net, x_T, cond, uncond, cfg_scale, timesteps, alphas, alphas_prev,
                             sqrt_one_minus_alphas, trace=self.trace, **kw)

    def sample_dpmpp(self, x_T, cond, uncond, cfg_scale, tables, control_scales=None, flags=0):
        self.dpmpp.append(dict(x_T=x_T, cond=cond, uncond=uncond, cfg_scale=cfg_scale, tables=tables, control_scales=control_scales,
                               flags=flags))
        return run_dpmpp_loop(self.dpmpp_step, self.net, x_T, cond, uncond, cfg_scale, tables)
