"""TEST INFRASTRUCTURE shared by tests/test_ancestral_loop_host.py (CPU) and tests/test_gpu_ancestral_loop.py (GPU): the device
ancestral loop and the device DDIM inversion restated in Python exactly as include/fgdm.h documents them (fgdm_sample_ancestral:
evaluate, update, the SAME step's blend; fgdm_ddim_encode: evaluate, then x = cx x + ce e), over a `step` function that stands for
ONE launch of the step kernel:

  ancestral_chain(k) / invert_chain(k)   the chain of existing kernels that one launch fuses, k = kernel_stubs (CPU) or
                                         fgdm_amd.engine (the HIP kernels): ancestral_step -> axpby + mask_blend, and
                                         cfg_combine -> axpby
  (the GPU tests pass a step that calls fgdm_op_ancestral_loop_step / fgdm_op_invert_loop_step instead)

and a stand-in engine (WalkEngine) whose sample_ancestral / ddim_encode run these loops on a closed-form network and record what
they were handed.  Never imported by the product."""
import torch


def ancestral_chain(k):
    """step(x, eps, (cr, crm1, c1, c2, std), noise, blend) -> x; blend: None or (mask, x0, q_noise, sqrt_ac_t, sqrt_one_minus_ac_t)"""
    def step(x, eps, coef, noise, blend):
        cr, crm1, c1, c2, std = coef
        xn = k.ancestral_step(x, eps, cr, crm1, c1, c2, std, noise if std != 0.0 else None)
        if blend is not None:
            mask, x0, qn, sa, s1m = blend
            xn = k.mask_blend(k.axpby(x0, sa, qn, s1m), xn, mask)
        return xn
    return step


def invert_chain(k):
    """step(x, ec, eu, cfg, cx, ce) -> x"""
    def step(x, ec, eu, cfg, cx, ce):
        e = ec if eu is None else k.cfg_combine(ec, eu, cfg)
        return k.axpby(x, cx, e, ce)
    return step


def run_ancestral_loop(step, net, x_T, cond, timesteps, tables, step_noise=None, mask=None, x0=None, q_noise=None, log_steps=()):
    """fgdm_sample_ancestral as its header comment describes it: everything in walk order"""
    x, logged = x_T, []
    for i, t in enumerate(timesteps):
        eps = net(x, torch.full((x.shape[0],), int(t), dtype=torch.long, device=x.device), cond)
        coef = tuple(float(tables[k][i]) for k in ('sqrt_recip_alphas_cumprod', 'sqrt_recipm1_alphas_cumprod', 'posterior_mean_coef1',
                                                   'posterior_mean_coef2', 'std'))
        blend = None if mask is None else (mask, x0, q_noise[i], float(tables['sqrt_alphas_cumprod_t'][i]),
                                           float(tables['sqrt_one_minus_alphas_cumprod_t'][i]))
        x = step(x, eps, coef, None if step_noise is None else step_noise[i], blend)
        if i in log_steps:
            logged.append(x)
    return x, (torch.stack(logged) if logged else None)


def run_encode_loop(step, net, x0, cond, uncond, cfg_scale, timesteps, cx, ce, log_steps=()):
    """fgdm_ddim_encode as its header comment describes it"""
    cfg_on = uncond is not None and cfg_scale != 1.0
    x, logged = x0, []
    for i, t in enumerate(timesteps):
        tt = torch.full((x.shape[0],), int(t), dtype=torch.long, device=x.device)
        if cfg_on:
            e_u, e_c = net(torch.cat([x] * 2), torch.cat([tt] * 2), torch.cat([uncond, cond])).chunk(2)
            x = step(x, e_c.contiguous(), e_u.contiguous(), cfg_scale, float(cx[i]), float(ce[i]))
        else:
            x = step(x, net(x, tt, cond), None, cfg_scale, float(cx[i]), float(ce[i]))
        if i in log_steps:
            logged.append(x)
    return x, (torch.stack(logged) if logged else None)


class WalkEngine:
    """An engine without networks: records what the model / the sampler hand to sample_ancestral / ddim_encode and runs the
    documented loops over `net` (x, t, context) -> eps with the given step functions."""
    has_vae, has_vae_encoder, has_clip = False, False, False

    def __init__(self, net, ancestral_step, invert_step, device='cpu'):
        self.net, self.ancestral_step, self.invert_step = net, ancestral_step, invert_step
        self.device = torch.device(device)
        self.ancestral, self.encodes = [], []

    def sample_ancestral(self, x_T, cond, timesteps, tables, control_scales=None, flags=0, **kw):
        self.ancestral.append(dict(kw, x_T=x_T, cond=cond, timesteps=list(timesteps), tables=tables, control_scales=control_scales,
                                   flags=flags))
        return run_ancestral_loop(self.ancestral_step, self.net, x_T, cond, timesteps, tables, **kw)

    def ddim_encode(self, x0, cond, uncond, cfg_scale, timesteps, cx, ce, log_steps=(), control_scales=None, flags=0):
        self.encodes.append(dict(x0=x0, cond=cond, uncond=uncond, cfg_scale=cfg_scale, timesteps=list(timesteps), cx=list(cx),
                                 ce=list(ce), log_steps=list(log_steps), control_scales=control_scales, flags=flags))
        return run_encode_loop(self.invert_step, self.net, x0, cond, uncond, cfg_scale, timesteps, cx, ce, log_steps)
