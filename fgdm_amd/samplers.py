"""Host-side mirrors of the reference samplers; same constructor / sample() / p_sample_* signatures.

  DDIMSampler         <- ldm/models/diffusion/ddim.py:13-412
  PLMSSampler         <- ldm/models/diffusion/plms.py:11-236
  ControlDDIMSampler  <- controlnet/cldm/ddim_hacked.py:10-317 (dict conditionings)

The loop stays on the host (callbacks, intermediates, kwargs pass-through keep their reference semantics);
every per-step tensor update is one fused HIP kernel (csrc/elementwise.hip) and every model evaluation is
`model.apply_model` -- for fgdm_amd.models.* that is the HIP engine.  CFG is evaluated as ONE 2B batch
(cat([uncond, cond])) like ddim.py:222-243; the ControlNet sampler's two sequential calls
(ddim_hacked.py:190-192) are batched the same way when both branches use the same hint (identical math).
Not carried over (dead or unreachable in the reference): inference_loss / return_conds / x2.

DDIMSampler / ControlDDIMSampler(model, device_loop=True) hand a whole sample() / ddim_sampling() / decode() to the engine's device
loop (fgdm_sample_ddim_ex) when nothing asked for needs the host between steps; the noise is drawn beforehand by the same calls in
the same order, so either route gives the same bits from the same generator state.  Everything else, and the default, is the
per-step loop below.  PLMSSampler and DPMSolverSampler take the same keyword and the same rule (_loop_plan / _loop_cond below) for
fgdm_sample_plms and fgdm_sample_dpmpp; the DPM-Solver++ coefficients of both routes come from dpmpp_tables.
ControlDDIMSampler.encode goes to fgdm_ddim_encode under the same rule, with the coefficients of encode_tables on both routes; the
ancestral loop's switch is the model's (fgdm_amd.models.LatentDiffusion(device_loop=True)).

device_noise=seed (DDIMSampler, ControlDDIMSampler, PLMSSampler; default None: everything above, bit for bit): the step noise and
q_sample's noise come from the engine's counter-based generator (fgdm_loop_noise_set / fgdm_randn, include/fgdm.h) instead of torch's.
The device route then draws nothing on the host and holds no [S, B,4,H,W] planes: the step kernels make the noise; the per-step
route takes the same numbers from Engine.randn at the same (stream, walk position, sample), so both routes still agree bit for bit.
x_T stays a torch draw.  noise_first_sample (default 0) is the global index of row 0: a rank's shard offset (fgdm_amd.dist).
"""
import numpy as np
import torch

from . import _lib
from . import engine as _k
from . import schedule


def _randn(shape, device):
    return torch.randn(shape, device=device)


# ---- the device loops (DDIM, PLMS, DPM-Solver++, the DPM-Solver program, ancestral, DDIM inversion): what they can take over
def _loop_cond(m, c, uc, cfg_on, sampler=None):
    """(ctx, uctx, flags, control_scales) the engine's loop needs for this conditioning of model `m`, after registering the
    hints as apply_model would -- or None: a conditioning the loop does not take (the per-step route then treats it as
    before).  sampler: the one whose _cat_cond would join the two branches of a ControlLDM (None: no sampler joins them)."""
    from . import _lib, models
    pair = _lib.FLAG_CFG_PAIRS if cfg_on else 0
    if isinstance(m, models.ControlLDM):
        if type(m).apply_model is not models.ControlLDM.apply_model:
            return None                                                   # a subclass with its own apply_model
        if cfg_on and not isinstance(sampler, ControlDDIMSampler):
            return None                                                   # only that sampler's _cat_cond joins dict conds
        if not isinstance(c, dict) or len(c.get('c_crossattn') or ()) != 1 or not torch.is_tensor(c['c_crossattn'][0]):
            return None
        if cfg_on and (not isinstance(uc, dict) or sampler._cat_cond(uc, c) is None):
            return None                                                   # branches that cannot share one batch: two calls per step
        hints = c.get('c_concat')
        flags = pair | (_lib.FLAG_ONLY_MID_CONTROL if m.only_mid_control else 0)
        ctx, uctx = c['c_crossattn'][0], uc['c_crossattn'][0] if cfg_on else None
        if hints is None:
            return ctx, uctx, flags | _lib.FLAG_NO_CONTROL, None
        if m.n_controlnets == 1:
            hints = [hints[0] if len(hints) == 1 else torch.cat(hints, 1)]
        if len(hints) != m.n_controlnets:
            return None
        for k, h in enumerate(hints):
            m.engine.set_hint(k, h)
        return ctx, uctx, flags, m._scales()
    if type(m).apply_model is not models.LatentDiffusion.apply_model or m.model.conditioning_key != 'crossattn':
        return None                                                       # hybrid c_concat, or a model with its own apply_model
    if not torch.is_tensor(c) or getattr(m.engine, '_conds_key', None) is not None:
        return None
    if cfg_on and (not torch.is_tensor(uc) or tuple(uc.shape) != tuple(c.shape)):
        return None
    return c, uc if cfg_on else None, _lib.FLAG_NO_CONTROL | pair, None


def _loop_plan(m, sampler, cond, uc, scales, mask, x0, img, host_hooks, kwargs, entry='sample_ddim_ex'):
    """None (per-step route), or the conditioning part of the device loop's arguments for model `m`.  sampler: the one that asks
    (its device_loop switch and dynamic threshold are honoured), or None: the caller has its own switch.  `scales`: the guidance
    scale of every step of the walk; host_hooks: whether anything asked for runs on the host between steps; entry: the engine
    method that runs the loop.  Draws no noise."""
    eng = getattr(m, 'engine', None)
    if (sampler is not None and not getattr(sampler, 'device_loop', False)) or eng is None or not hasattr(eng, entry) or host_hooks or kwargs:
        return None
    if getattr(m, 'split_input_params', None) is not None or getattr(sampler, '_dyn', None) is not None:
        return None
    if getattr(m, 'parameterization', 'eps') != 'eps' or not hasattr(m, '_host') or img.dim() != 4 or img.shape[1] != 4:
        return None
    on = [uc is not None and s != 1. for s in scales]
    if any(on) != all(on):
        return None                 # a ucg_schedule that is 1 at some steps: those steps run without the unconditional half
    if mask is not None and (x0 is None or tuple(x0.shape) != tuple(img.shape)):
        return None
    return _loop_cond(m, cond, uc, all(on), sampler)


class _SamplerBase:
    def __init__(self, model, schedule="linear", device_noise=None, **kwargs):
        self.model = model
        self.ddpm_num_timesteps = model.num_timesteps
        self.schedule = schedule
        self.device_noise = device_noise        # None: torch's generator; a seed: the engine's generator (module docstring)
        self.noise_first_sample = 0
        self._noise_pos = 0                     # walk position of the step the per-step route is in

    def _generated(self, stream, shape, device, repeat=False, temperature=1.):
        """the per-step route's draw at the walk position it is in, from the engine's generator (device_noise is a seed)"""
        return _k.randn(self.device_noise, stream, getattr(self, '_noise_pos', 0), shape, getattr(self, 'noise_first_sample', 0), repeat, temperature, device=device)

    def register_buffer(self, name, attr):
        if isinstance(attr, torch.Tensor) and attr.device != torch.device(self.model.device):
            attr = attr.to(self.model.device)
        setattr(self, name, attr)

    # ddim.py:26-55
    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0., verbose=True):
        self.ddim_timesteps = schedule.ddim_timesteps(ddim_discretize, ddim_num_steps, self.ddpm_num_timesteps)
        if verbose:
            print(f'Selected timesteps for ddim sampler: {self.ddim_timesteps}')
        ac = self.model.alphas_cumprod
        assert ac.shape[0] == self.ddpm_num_timesteps, 'alphas have to be defined for each timestep'
        f32 = lambda v: torch.as_tensor(v).clone().detach().to(torch.float32).to(self.model.device)
        ac_h = ac.detach().float().cpu()
        self.register_buffer('betas', f32(self.model.betas))
        self.register_buffer('alphas_cumprod', f32(ac))
        self.register_buffer('alphas_cumprod_prev', f32(self.model.alphas_cumprod_prev))
        self.register_buffer('sqrt_alphas_cumprod', f32(torch.sqrt(ac_h)))
        self.register_buffer('sqrt_one_minus_alphas_cumprod', f32(torch.sqrt(1. - ac_h)))
        self.register_buffer('log_one_minus_alphas_cumprod', f32(torch.log(1. - ac_h)))
        self.register_buffer('sqrt_recip_alphas_cumprod', f32(torch.sqrt(1. / ac_h)))
        self.register_buffer('sqrt_recipm1_alphas_cumprod', f32(torch.sqrt(1. / ac_h - 1)))
        sig, a, ap, s1m = schedule.ddim_tables(ac_h.numpy(), self.ddim_timesteps, ddim_eta)
        if verbose:
            print(f'Selected alphas for ddim sampler: a_t: {a}; a_(t-1): {ap}')
            print(f'For the chosen value of eta, which is {ddim_eta}, this results in the following sigma_t '
                  f'schedule for ddim sampler {sig}')
        self.ddim_sigmas, self.ddim_alphas, self.ddim_alphas_prev, self.ddim_sqrt_one_minus_alphas = sig, a, ap, s1m
        acp_h = self.model.alphas_cumprod_prev.detach().float().cpu()
        self.register_buffer('ddim_sigmas_for_original_num_steps',
                             ddim_eta * torch.sqrt((1 - acp_h) / (1 - ac_h) * (1 - ac_h / acp_h)))

    def _tables(self, use_original_steps):
        """(alphas, alphas_prev, sqrt_one_minus_alphas, sigmas) as host float arrays (ddim.py:249-252)."""
        if not use_original_steps:
            return self.ddim_alphas, self.ddim_alphas_prev, self.ddim_sqrt_one_minus_alphas, self.ddim_sigmas
        h = lambda v: v.detach().float().cpu().numpy()
        return (h(self.model.alphas_cumprod), h(self.model.alphas_cumprod_prev),
                h(self.model.sqrt_one_minus_alphas_cumprod), h(self.ddim_sigmas_for_original_num_steps))

    @staticmethod
    def _batch_of(conditioning):
        if isinstance(conditioning, dict):
            v = conditioning[list(conditioning.keys())[0]]
            while isinstance(v, (list, tuple)):
                v = v[0]
            return v.shape[0]
        return conditioning.shape[0]

    # ---- model evaluation with classifier-free guidance; returns (e_cond, e_uncond_or_None)
    def _eval_pair(self, x, t, c, uc, scale, **kwargs):
        if uc is None or scale == 1.:
            return self.model.apply_model(x, t, c, **kwargs), None
        x_in, t_in = torch.cat([x] * 2), torch.cat([t] * 2)
        c_in = self._batched_cond(uc, c)
        if c_in is None:        # conditionings that cannot share one batch: two calls (ddim_hacked.py:190-191)
            return self.model.apply_model(x, t, c, **kwargs), self.model.apply_model(x, t, uc, **kwargs)
        # cfg_pairs: rows b and b + B of this batch differ only in the context (lets the engine share the network prefix).
        # The hint is understood by this repo's mirrors only: any other `model` (e.g. the reference's LatentDiffusion,
        # which forwards **kwargs into UNetModel.forward) is called exactly as the reference calls it.
        if getattr(self.model, 'engine', None) is not None:
            kwargs = dict(kwargs, cfg_pairs=True)
        e_u, e_c = self.model.apply_model(x_in, t_in, c_in, **kwargs).chunk(2)
        return e_c.contiguous(), e_u.contiguous()

    @staticmethod
    def _cat_cond(uc, c):
        return torch.cat([uc, c])

    @staticmethod
    def _leaves(c, out):
        if torch.is_tensor(c):
            out.append(c)
        elif isinstance(c, dict):
            for k in sorted(c):
                _SamplerBase._leaves(c[k], out)
        elif isinstance(c, (list, tuple)):
            for v in c:
                _SamplerBase._leaves(v, out)
        return out

    def _batched_cond(self, uc, c):
        """cat([uc, c]) is loop-invariant: build it once per (uc, c) pair and hand the SAME tensor object to every step,
        so the engine can keep the context's K/V projections (Engine.apply_model).  The memo holds the source tensors, so
        their ids cannot be recycled, and is invalidated by any in-place modification (_version)."""
        leaves = self._leaves(uc, []) + self._leaves(c, [])
        key = tuple((id(t), t._version) for t in leaves)
        memo = getattr(self, '_cin_memo', None)
        if memo is not None and memo[0] == key:
            return memo[2]
        c_in = self._cat_cond(uc, c)
        self._cin_memo = (key, leaves, c_in)
        return c_in

    def _x_prev(self, x, e_cond, e_uncond, scale, index, tabs, temperature, noise_dropout, repeat_noise,
                want_pred_x0=True):
        alphas, alphas_prev, s1m, sigmas = tabs
        sigma = float(sigmas[index])
        # the reference draws noise_like(x.shape) on EVERY step, also when sigma == 0 (ddim.py:265); drawing it
        # keeps the generator stream aligned with the reference (matters when q_sample also draws: mask blending)
        shape = (1, *x.shape[1:]) if repeat_noise else x.shape
        generated = getattr(self, 'device_noise', None) is not None
        noise = None if generated else _randn(shape, x.device)
        if sigma == 0.0:
            noise = None
        elif generated:                                           # repeat_noise and temperature are the generator's
            noise = self._generated(_lib.NOISE_STREAM_STEP, x.shape, x.device, repeat_noise, temperature)
            if noise_dropout > 0.:
                noise = torch.nn.functional.dropout(noise, p=noise_dropout)
        else:
            if repeat_noise:
                noise = noise.expand_as(x).contiguous()
            if temperature != 1.:
                noise = noise * temperature                       # rare options: plain tensor ops on the noise only
            if noise_dropout > 0.:
                noise = torch.nn.functional.dropout(noise, p=noise_dropout)
        return _k.ddim_step(x.contiguous(), e_cond, e_uncond, scale, float(alphas[index]), float(alphas_prev[index]),
                            sigma, float(s1m[index]), noise, want_pred_x0)

    def _blend_mask(self, img, mask, x0, ts):
        if getattr(self, 'device_noise', None) is None:
            img_orig = self.model.q_sample(x0, ts)
        else:
            img_orig = self.model.q_sample(x0, ts, self._generated(_lib.NOISE_STREAM_Q, x0.shape, x0.device))
        m = mask.to(img.dtype).expand_as(img).contiguous()
        return _k.mask_blend(img_orig.contiguous(), img.contiguous(), m)

    def stochastic_encode(self, x0, t, use_original_steps=False, noise=None):
        """q(x_t | x_0) at (ddim) index t (ddim.py:379-393)."""
        if use_original_steps:
            sa, s1m = self.sqrt_alphas_cumprod.cpu().numpy(), self.sqrt_one_minus_alphas_cumprod.cpu().numpy()
        else:
            sa, s1m = np.sqrt(self.ddim_alphas), self.ddim_sqrt_one_minus_alphas
        noise = torch.randn_like(x0) if noise is None else noise
        ti = np.asarray(t.detach().cpu())
        assert (ti == ti.flat[0]).all(), 'one encode index per call'
        return _k.axpby(x0.contiguous(), float(sa[ti.flat[0]]), noise.contiguous(), float(s1m[ti.flat[0]]))


    def _mask_kw(self, mask, x0, qn, img, timesteps):
        """the mask group of a device loop's arguments ({} without a mask); qn: q_sample's noise of every step, already drawn
        (None: the armed engine makes it)"""
        if mask is None:
            return {}
        h = self.model._host
        return dict(mask=mask.to(img.dtype).expand_as(img).contiguous(), x0=x0, q_noise=None if qn is None else torch.stack(qn),
                    sqrt_alphas_cumprod_t=[h['sqrt_alphas_cumprod'][int(t)] for t in timesteps],
                    sqrt_one_minus_alphas_cumprod_t=[h['sqrt_one_minus_alphas_cumprod'][int(t)] for t in timesteps])

    @staticmethod
    def _log_steps(total_steps, log_every_t):
        """walk positions whose x_prev / pred_x0 the loops log: `index % log_every_t == 0 or index == total_steps - 1`"""
        return [i for i in range(total_steps) if (total_steps - i - 1) % log_every_t == 0 or i == 0]


class DDIMSampler(_SamplerBase):
    def __init__(self, model, schedule="linear", device_loop=False, **kwargs):
        super().__init__(model, schedule, **kwargs)
        self.device_loop = bool(device_loop)

    def _device_loop(self, plan, img, timesteps, tabs, scales, mask, x0, temperature, log_steps):
        """Draw the walk's noise as the per-step route would (per step: q_sample's if there is a mask, then the step's, which is
        drawn and dropped where sigma is 0), then one engine call.  timesteps / tabs in ddim_timesteps order, S entries."""
        ctx, uctx, flags, control_scales = plan
        S = len(timesteps)
        alphas, alphas_prev, s1m, sigmas = (np.asarray(t)[:S] for t in tabs)
        cfg_on = uctx is not None
        if getattr(self, 'device_noise', None) is not None:      # nothing is drawn: the armed engine makes both streams in its step kernels
            with self.model.engine.loop_noise(self.device_noise, self.noise_first_sample, 0, temperature):
                return self.model.engine.sample_ddim_ex(img, ctx, uctx, scales[0] if cfg_on else 1.0, [int(t) for t in timesteps], alphas,
                                                        alphas_prev, s1m, sigmas=sigmas, cfg_scales=scales if cfg_on else None,
                                                        log_steps=log_steps, control_scales=control_scales, flags=flags,
                                                        **self._mask_kw(mask, x0, None, img, timesteps))
        qn, sn = [], []
        for i in range(S):
            if mask is not None:
                qn.append(torch.randn_like(x0))                               # q_sample(x0, ts)
            noise = _randn(img.shape, img.device)
            if float(sigmas[S - 1 - i]) != 0.0 and temperature != 1.:
                noise = noise * temperature
            if sigmas.any():
                sn.append(noise)
        kw = self._mask_kw(mask, x0, qn, img, timesteps)
        return self.model.engine.sample_ddim_ex(img, ctx, uctx, scales[0] if cfg_on else 1.0, [int(t) for t in timesteps], alphas,
                                                alphas_prev, s1m, sigmas=sigmas, cfg_scales=scales if cfg_on else None,
                                                step_noise=torch.stack(sn) if sn else None, log_steps=log_steps,
                                                control_scales=control_scales, flags=flags, **kw)

    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None,
               img_callback=None, quantize_x0=False, eta=0., mask=None, x0=None, temperature=1., noise_dropout=0.,
               score_corrector=None, corrector_kwargs=None, verbose=True, x_T=None, log_every_t=100,
               unconditional_guidance_scale=1., unconditional_conditioning=None, inference_loss=False, **kwargs):
        if conditioning is not None:
            cbs = self._batch_of(conditioning)
            if cbs != batch_size:
                print(f"Warning: Got {cbs} conditionings but batch-size is {batch_size}")
        self.make_schedule(ddim_num_steps=S, ddim_eta=eta, verbose=verbose)
        C, H, W = shape
        size = (batch_size, C, H, W)
        if verbose:
            print(f'Data shape for DDIM sampling is {size}, eta {eta}')
        return self.ddim_sampling(conditioning, size, callback=callback, img_callback=img_callback,
                                  quantize_denoised=quantize_x0, mask=mask, x0=x0, ddim_use_original_steps=False,
                                  noise_dropout=noise_dropout, temperature=temperature,
                                  score_corrector=score_corrector, corrector_kwargs=corrector_kwargs, x_T=x_T,
                                  log_every_t=log_every_t, unconditional_guidance_scale=unconditional_guidance_scale,
                                  unconditional_conditioning=unconditional_conditioning,
                                  inference_loss=inference_loss, **kwargs)

    def ddim_sampling(self, cond, shape, x_T=None, ddim_use_original_steps=False, callback=None, timesteps=None,
                      quantize_denoised=False, mask=None, x0=None, img_callback=None, log_every_t=100,
                      temperature=1., noise_dropout=0., score_corrector=None, corrector_kwargs=None,
                      unconditional_guidance_scale=1., unconditional_conditioning=None, inference_loss=False,
                      **kwargs):
        device = self.model.betas.device
        b = shape[0]
        img = _randn(shape, device) if x_T is None else x_T.to(device, torch.float32)
        if timesteps is None:
            timesteps = self.ddpm_num_timesteps if ddim_use_original_steps else self.ddim_timesteps
        elif not ddim_use_original_steps:
            n = self.ddim_timesteps.shape[0]
            timesteps = self.ddim_timesteps[:int(min(timesteps / n, 1) * n) - 1]
        intermediates = {'x_inter': [img], 'pred_x0': [img]}
        time_range = list(reversed(range(0, timesteps))) if ddim_use_original_steps else np.flip(timesteps)
        total_steps = timesteps if ddim_use_original_steps else timesteps.shape[0]
        ucg = getattr(self, '_ucg', None)
        scales = [unconditional_guidance_scale if ucg is None else ucg[i] for i in range(total_steps)] \
            if ucg is None or len(ucg) >= total_steps else None
        hooks = bool(callback or img_callback or score_corrector is not None or noise_dropout > 0. or quantize_denoised
                     or inference_loss)
        plan = None if scales is None or total_steps < 1 else \
            _loop_plan(self.model, self, cond, unconditional_conditioning, scales, mask, x0, img, hooks, kwargs)
        if plan is not None:
            log_steps = self._log_steps(total_steps, log_every_t)
            img, x_inter, pred = self._device_loop(plan, img, list(reversed([int(t) for t in time_range])),
                                                   self._tables(ddim_use_original_steps), scales, mask, x0, temperature, log_steps)
            intermediates['x_inter'] += list(x_inter)
            intermediates['pred_x0'] += list(pred)
            return img, intermediates
        for i, step in enumerate(time_range):
            index = total_steps - i - 1
            self._noise_pos = i
            ts = torch.full((b,), int(step), device=device, dtype=torch.long)
            if mask is not None:
                assert x0 is not None
                img = self._blend_mask(img, mask, x0, ts)
            img, pred_x0 = self.p_sample_ddim(img, cond, ts, index=index, use_original_steps=ddim_use_original_steps,
                                              quantize_denoised=quantize_denoised, temperature=temperature,
                                              noise_dropout=noise_dropout, score_corrector=score_corrector,
                                              corrector_kwargs=corrector_kwargs,
                                              unconditional_guidance_scale=unconditional_guidance_scale,
                                              unconditional_conditioning=unconditional_conditioning, i=i,
                                              inference_loss=inference_loss, **kwargs)
            if callback:
                callback(i)
            if img_callback:
                img_callback(pred_x0, i)
            if index % log_every_t == 0 or index == total_steps - 1:
                intermediates['x_inter'].append(img)
                intermediates['pred_x0'].append(pred_x0)
        return img, intermediates

    def p_sample_ddim(self, x, c, t, index, repeat_noise=False, use_original_steps=False, quantize_denoised=False,
                      temperature=1., noise_dropout=0., score_corrector=None, corrector_kwargs=None,
                      unconditional_guidance_scale=1., unconditional_conditioning=None, i=0, inference_loss=False,
                      **kwargs):
        if inference_loss or kwargs.get('return_conds'):
            raise NotImplementedError('attention-alignment guidance / joint condition update need a model with a '
                                      'tuple output; no shipped model provides one (dead code in the reference)')
        if quantize_denoised:
            raise NotImplementedError('quantize_denoised needs a VQ first stage (not part of the latent-diffusion path)')
        uc, scale = unconditional_conditioning, unconditional_guidance_scale
        e_u = None
        if uc is None or scale == 1.:
            e_c = self.model.apply_model(x, t, c, **kwargs)
        elif 'composable_diffusion' in kwargs:                      # ddim.py:204-212
            kw = {k: v for k, v in kwargs.items() if k != 'composable_diffusion'}
            n = kwargs['composable_diffusion'] + 1
            out = self.model.apply_model(torch.cat([x] * n), torch.cat([t] * n), torch.cat([uc, c]), **kw)
            e_c = _k.axpby(out[:1].contiguous(), float(2 - n), None, 0.0)          # e_u + sum_k (e_k - e_u)
            for k in range(1, n):
                e_c = _k.axpby(e_c, 1.0, out[k:k + 1].contiguous(), 1.0)
        elif 'augmented_conditoning' in kwargs:                     # ddim.py:213-220 (sic)
            kw = {k: v for k, v in kwargs.items() if k not in ('augmented_conditoning', 'ac')}
            e_un, e_t, e_ac = self.model.apply_model(torch.cat([x] * 3), torch.cat([t] * 3),
                                                     torch.cat([uc, c, kwargs['ac']]), **kw).chunk(3)
            e_c = _k.cfg_combine(e_t.contiguous(), e_ac.contiguous(), scale)
            e_u = e_un.contiguous()
        else:
            e_c, e_u = self._eval_pair(x, t, c, uc, scale, **kwargs)
        if score_corrector is not None:
            assert self.model.parameterization == "eps"
            e_c = _k.cfg_combine(e_c, e_u, scale) if e_u is not None else e_c
            e_c, e_u = score_corrector.modify_score(self.model, e_c, x, t, c, **(corrector_kwargs or {})), None
        return self._x_prev(x, e_c, e_u, scale, index, self._tables(use_original_steps), temperature,
                            noise_dropout, repeat_noise)

    def decode(self, x_latent, cond, t_start, unconditional_guidance_scale=1.0, unconditional_conditioning=None,
               use_original_steps=False, callback=None):
        timesteps = np.arange(self.ddpm_num_timesteps) if use_original_steps else self.ddim_timesteps
        timesteps = timesteps[:t_start]
        total_steps = timesteps.shape[0]
        x_dec = x_latent
        # (ControlDDIMSampler.p_sample_ddim reads a ucg_schedule left by an earlier ddim_sampling at i = 0: per-step route)
        plan = None if total_steps < 1 or getattr(self, '_ucg', None) is not None else \
            _loop_plan(self.model, self, cond, unconditional_conditioning, [unconditional_guidance_scale] * total_steps, None, None, x_latent,
                            bool(callback), {})
        if plan is not None:
            return self._device_loop(plan, x_latent, [int(t) for t in timesteps], self._tables(use_original_steps),
                                     [unconditional_guidance_scale] * total_steps, None, None, 1., ())[0]
        for i, step in enumerate(np.flip(timesteps)):
            index = total_steps - i - 1
            self._noise_pos = i
            ts = torch.full((x_latent.shape[0],), int(step), device=x_latent.device, dtype=torch.long)
            x_dec, _ = self.p_sample_ddim(x_dec, cond, ts, index=index, use_original_steps=use_original_steps,
                                          unconditional_guidance_scale=unconditional_guidance_scale,
                                          unconditional_conditioning=unconditional_conditioning)
            if callback:
                callback(i)
        return x_dec


class PLMSSampler(_SamplerBase):
    def __init__(self, model, schedule="linear", device_loop=False, **kwargs):
        super().__init__(model, schedule, **kwargs)
        self.device_loop = bool(device_loop)

    def _device_loop(self, plan, img, timesteps, tabs, scale, mask, x0, log_steps):
        """Draw what the per-step route draws, in its order -- per step q_sample's noise if there is a mask, then one noise per
        _x_prev call (two in the first step, all dropped: sigma is 0) -- then one engine call (fgdm_sample_plms)."""
        ctx, uctx, flags, control_scales = plan
        S = len(timesteps)
        alphas, alphas_prev, s1m = (np.asarray(t)[:S] for t in tabs[:3])
        if getattr(self, 'device_noise', None) is not None:      # nothing is drawn: the armed engine makes q_sample's noise in its step kernel
            with self.model.engine.loop_noise(self.device_noise, self.noise_first_sample):
                return self.model.engine.sample_plms(img, ctx, uctx, scale if uctx is not None else 1.0, [int(t) for t in timesteps],
                                                     alphas, alphas_prev, s1m, log_steps=log_steps, control_scales=control_scales,
                                                     flags=flags, **self._mask_kw(mask, x0, None, img, timesteps))
        qn = []
        for i in range(S):
            if mask is not None:
                qn.append(torch.randn_like(x0))                               # q_sample(x0, ts)
            for _ in range(2 if i == 0 else 1):
                _randn(img.shape, img.device)
        kw = self._mask_kw(mask, x0, qn, img, timesteps)
        return self.model.engine.sample_plms(img, ctx, uctx, scale if uctx is not None else 1.0, [int(t) for t in timesteps],
                                             alphas, alphas_prev, s1m, log_steps=log_steps, control_scales=control_scales,
                                             flags=flags, **kw)

    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0., verbose=True):
        if ddim_eta != 0:
            raise ValueError('ddim_eta must be 0 for PLMS')       # plms.py:25-26
        super().make_schedule(ddim_num_steps, ddim_discretize, ddim_eta, verbose)

    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None,
               img_callback=None, quantize_x0=False, eta=0., mask=None, x0=None, temperature=1., noise_dropout=0.,
               score_corrector=None, corrector_kwargs=None, verbose=True, x_T=None, log_every_t=100,
               unconditional_guidance_scale=1., unconditional_conditioning=None, **kwargs):
        if conditioning is not None:
            cbs = self._batch_of(conditioning)
            if cbs != batch_size:
                print(f"Warning: Got {cbs} conditionings but batch-size is {batch_size}")
        self.make_schedule(ddim_num_steps=S, ddim_eta=eta, verbose=verbose)
        C, H, W = shape
        size = (batch_size, C, H, W)
        if verbose:
            print(f'Data shape for PLMS sampling is {size}')
        return self.plms_sampling(conditioning, size, callback=callback, img_callback=img_callback,
                                  quantize_denoised=quantize_x0, mask=mask, x0=x0, ddim_use_original_steps=False,
                                  noise_dropout=noise_dropout, temperature=temperature,
                                  score_corrector=score_corrector, corrector_kwargs=corrector_kwargs, x_T=x_T,
                                  log_every_t=log_every_t, unconditional_guidance_scale=unconditional_guidance_scale,
                                  unconditional_conditioning=unconditional_conditioning)

    def plms_sampling(self, cond, shape, x_T=None, ddim_use_original_steps=False, callback=None, timesteps=None,
                      quantize_denoised=False, mask=None, x0=None, img_callback=None, log_every_t=100,
                      temperature=1., noise_dropout=0., score_corrector=None, corrector_kwargs=None,
                      unconditional_guidance_scale=1., unconditional_conditioning=None):
        device = self.model.betas.device
        b = shape[0]
        img = _randn(shape, device) if x_T is None else x_T.to(device, torch.float32)
        if timesteps is None:
            timesteps = self.ddpm_num_timesteps if ddim_use_original_steps else self.ddim_timesteps
        elif not ddim_use_original_steps:
            n = self.ddim_timesteps.shape[0]
            timesteps = self.ddim_timesteps[:int(min(timesteps / n, 1) * n) - 1]
        intermediates = {'x_inter': [img], 'pred_x0': [img]}
        time_range = list(reversed(range(0, timesteps))) if ddim_use_original_steps else np.flip(timesteps)
        total_steps = timesteps if ddim_use_original_steps else timesteps.shape[0]
        hooks = bool(callback or img_callback or score_corrector is not None or noise_dropout > 0. or quantize_denoised)
        tabs = self._tables(ddim_use_original_steps)
        plan = None if total_steps < 1 or np.asarray(tabs[3])[:total_steps].any() else \
            _loop_plan(self.model, self, cond, unconditional_conditioning, [unconditional_guidance_scale] * total_steps, mask, x0, img, hooks, {},
                            entry='sample_plms')
        if plan is not None:
            img, x_inter, pred = self._device_loop(plan, img, list(reversed([int(t) for t in time_range])), tabs,
                                                   unconditional_guidance_scale, mask, x0, self._log_steps(total_steps, log_every_t))
            intermediates['x_inter'] += list(x_inter)
            intermediates['pred_x0'] += list(pred)
            return img, intermediates
        old_eps = []
        for i, step in enumerate(time_range):
            index = total_steps - i - 1
            ts = torch.full((b,), int(step), device=device, dtype=torch.long)
            ts_next = torch.full((b,), int(time_range[min(i + 1, len(time_range) - 1)]), device=device, dtype=torch.long)
            self._noise_pos = i
            if mask is not None:
                assert x0 is not None
                img = self._blend_mask(img, mask, x0, ts)
            img, pred_x0, e_t = self.p_sample_plms(img, cond, ts, index=index, use_original_steps=ddim_use_original_steps,
                                                   quantize_denoised=quantize_denoised, temperature=temperature,
                                                   noise_dropout=noise_dropout, score_corrector=score_corrector,
                                                   corrector_kwargs=corrector_kwargs,
                                                   unconditional_guidance_scale=unconditional_guidance_scale,
                                                   unconditional_conditioning=unconditional_conditioning,
                                                   old_eps=old_eps, t_next=ts_next)
            old_eps.append(e_t)
            if len(old_eps) >= 4:
                old_eps.pop(0)
            if callback:
                callback(i)
            if img_callback:
                img_callback(pred_x0, i)
            if index % log_every_t == 0 or index == total_steps - 1:
                intermediates['x_inter'].append(img)
                intermediates['pred_x0'].append(pred_x0)
        return img, intermediates

    def p_sample_plms(self, x, c, t, index, repeat_noise=False, use_original_steps=False, quantize_denoised=False,
                      temperature=1., noise_dropout=0., score_corrector=None, corrector_kwargs=None,
                      unconditional_guidance_scale=1., unconditional_conditioning=None, old_eps=None, t_next=None):
        if quantize_denoised:
            raise NotImplementedError('quantize_denoised needs a VQ first stage')
        uc, scale = unconditional_conditioning, unconditional_guidance_scale
        tabs = self._tables(use_original_steps)

        def model_output(xx, tt):
            e_c, e_u = self._eval_pair(xx, tt, c, uc, scale)
            e = _k.cfg_combine(e_c, e_u, scale) if e_u is not None else e_c
            if score_corrector is not None:
                assert self.model.parameterization == "eps"
                e = score_corrector.modify_score(self.model, e, xx, tt, c, **(corrector_kwargs or {}))
            return e

        step = lambda e: self._x_prev(x, e, None, 1.0, index, tabs, temperature, noise_dropout, repeat_noise)
        e_t = model_output(x, t)
        if len(old_eps) == 0:            # pseudo improved Euler (plms.py:219-223): second evaluation at t_next
            x_prev, _ = step(e_t)
            e_prime = _k.axpby(e_t, 0.5, model_output(x_prev, t_next), 0.5)
        else:                            # Adams-Bashforth 2 / 3 / 4 (plms.py:224-232)
            e_prime = _k.plms_combine(e_t, old_eps)
        x_prev, pred_x0 = step(e_prime)
        return x_prev, pred_x0, e_t


def encode_tables(a_next, a_cur):
    """The coefficients of DDIM inversion's x_next = cx x + ce e_t (ddim_hacked.py:262-266) for every step, from the fp32 alphas of
    the step's target and source timestep: cx = sqrt(a_next / a_cur) and ce = sqrt(a_next) (sqrt(1 / a_next - 1) - sqrt(1 / a_cur - 1)),
    evaluated in numpy float32 scalars.  Both routes of ControlDDIMSampler.encode take them from here."""
    f32 = np.float32
    a_next, a_cur = np.asarray(a_next, dtype=f32), np.asarray(a_cur, dtype=f32)
    cx, ce = [], []
    for i in range(len(a_next)):
        cx.append(float(np.sqrt(a_next[i] / a_cur[i])))
        ce.append(float(np.sqrt(a_next[i]) * (np.sqrt(f32(1) / a_next[i] - f32(1)) - np.sqrt(f32(1) / a_cur[i] - f32(1)))))
    return cx, ce


class ControlDDIMSampler(DDIMSampler):
    """controlnet/cldm/ddim_hacked.py: conditionings are dicts {'c_concat': [hint] | None, 'c_crossattn': [ctx]}."""

    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None,
               img_callback=None, quantize_x0=False, eta=0., mask=None, x0=None, temperature=1., noise_dropout=0.,
               score_corrector=None, corrector_kwargs=None, verbose=True, x_T=None, log_every_t=100,
               unconditional_guidance_scale=1., unconditional_conditioning=None, dynamic_threshold=None,
               ucg_schedule=None, **kwargs):
        if conditioning is not None:
            cbs = self._batch_of(conditioning)
            if cbs != batch_size:
                print(f"Warning: Got {cbs} conditionings but batch-size is {batch_size}")
        self.make_schedule(ddim_num_steps=S, ddim_eta=eta, verbose=verbose)
        C, H, W = shape
        size = (batch_size, C, H, W)
        if verbose:
            print(f'Data shape for DDIM sampling is {size}, eta {eta}')
        return self.ddim_sampling(conditioning, size, callback=callback, img_callback=img_callback,
                                  quantize_denoised=quantize_x0, mask=mask, x0=x0, ddim_use_original_steps=False,
                                  noise_dropout=noise_dropout, temperature=temperature,
                                  score_corrector=score_corrector, corrector_kwargs=corrector_kwargs, x_T=x_T,
                                  log_every_t=log_every_t, unconditional_guidance_scale=unconditional_guidance_scale,
                                  unconditional_conditioning=unconditional_conditioning,
                                  dynamic_threshold=dynamic_threshold, ucg_schedule=ucg_schedule)

    def ddim_sampling(self, cond, shape, x_T=None, ddim_use_original_steps=False, callback=None, timesteps=None,
                      quantize_denoised=False, mask=None, x0=None, img_callback=None, log_every_t=100,
                      temperature=1., noise_dropout=0., score_corrector=None, corrector_kwargs=None,
                      unconditional_guidance_scale=1., unconditional_conditioning=None, dynamic_threshold=None,
                      ucg_schedule=None):
        self._ucg = ucg_schedule
        self._dyn = dynamic_threshold
        if ucg_schedule is not None:
            n = self.ddpm_num_timesteps if ddim_use_original_steps else len(self.ddim_timesteps)
            assert timesteps is not None or len(ucg_schedule) == n
        return super().ddim_sampling(cond, shape, x_T=x_T, ddim_use_original_steps=ddim_use_original_steps,
                                     callback=callback, timesteps=timesteps, quantize_denoised=quantize_denoised,
                                     mask=mask, x0=x0, img_callback=img_callback, log_every_t=log_every_t,
                                     temperature=temperature, noise_dropout=noise_dropout,
                                     score_corrector=score_corrector, corrector_kwargs=corrector_kwargs,
                                     unconditional_guidance_scale=unconditional_guidance_scale,
                                     unconditional_conditioning=unconditional_conditioning)

    def p_sample_ddim(self, x, c, t, index, repeat_noise=False, use_original_steps=False, quantize_denoised=False,
                      temperature=1., noise_dropout=0., score_corrector=None, corrector_kwargs=None,
                      unconditional_guidance_scale=1., unconditional_conditioning=None, dynamic_threshold=None,
                      i=0, inference_loss=False, **kwargs):
        if dynamic_threshold is not None or getattr(self, '_dyn', None) is not None:
            raise NotImplementedError()                              # ddim_hacked.py:222-223
        if getattr(self, '_ucg', None) is not None:                 # ddim_hacked.py:159-161
            unconditional_guidance_scale = self._ucg[i]
        if self.model.parameterization == "v":
            raise NotImplementedError('v-parameterization is not used by cldm_v15 configs')
        return super().p_sample_ddim(x, c, t, index, repeat_noise=repeat_noise, use_original_steps=use_original_steps,
                                     quantize_denoised=quantize_denoised, temperature=temperature,
                                     noise_dropout=noise_dropout, score_corrector=score_corrector,
                                     corrector_kwargs=corrector_kwargs,
                                     unconditional_guidance_scale=unconditional_guidance_scale,
                                     unconditional_conditioning=unconditional_conditioning)

    def encode(self, x0, c, t_enc, use_original_steps=False, return_intermediates=None,
               unconditional_guidance_scale=1.0, unconditional_conditioning=None, callback=None):
        """DDIM inversion x_0 -> x_{t_enc} (ddim_hacked.py:234-279); requires make_schedule() first.  device_loop=True and no
        callback: one engine call (fgdm_ddim_encode) under the rule of _loop_plan, with the same bits."""
        timesteps = np.arange(self.ddpm_num_timesteps) if use_original_steps else self.ddim_timesteps
        assert t_enc <= timesteps.shape[0]
        if use_original_steps:
            a_next = self.alphas_cumprod[:t_enc].detach().cpu().numpy().astype(np.float32)
            a_cur = self.alphas_cumprod_prev[:t_enc].detach().cpu().numpy().astype(np.float32)
        else:
            a_next = np.asarray(self.ddim_alphas[:t_enc], dtype=np.float32)
            a_cur = np.asarray(self.ddim_alphas_prev[:t_enc], dtype=np.float32)
        cx, ce = encode_tables(a_next, a_cur)
        x_next = x0
        intermediates, inter_steps = [], []
        scale, uc = unconditional_guidance_scale, unconditional_conditioning
        plan = None
        if t_enc >= 1 and (scale == 1. or uc is not None):
            plan = _loop_plan(self.model, self, c, uc if scale != 1. else None, [scale] * t_enc, None, None, x0, bool(callback), {},
                                   entry='ddim_encode')
        if plan is not None:
            ctx, uctx, flags, control_scales = plan
            inter_steps = [i for i in range(t_enc) if return_intermediates and (
                (i % (t_enc // return_intermediates) == 0 and i < t_enc - 1) or i >= t_enc - 2)]
            x_next, x_inter = self.model.engine.ddim_encode(x0, ctx, uctx, scale if uctx is not None else 1.0,
                                                            [int(t) for t in timesteps[:t_enc]], cx, ce, log_steps=inter_steps,
                                                            control_scales=control_scales, flags=flags)
            intermediates = list(x_inter) if inter_steps else []
        else:
            for i in range(t_enc):
                t = torch.full((x0.shape[0],), int(timesteps[i]), device=self.model.device, dtype=torch.long)
                if unconditional_guidance_scale == 1.:
                    e = self.model.apply_model(x_next, t, c)
                else:
                    assert unconditional_conditioning is not None
                    e_c, e_u = self._eval_pair(x_next, t, c, unconditional_conditioning, unconditional_guidance_scale)
                    e = _k.cfg_combine(e_c, e_u, unconditional_guidance_scale) if e_u is not None else e_c
                x_next = _k.axpby(x_next.contiguous(), cx[i], e, ce[i])
                if return_intermediates and i % (t_enc // return_intermediates) == 0 and i < t_enc - 1:
                    intermediates.append(x_next)
                    inter_steps.append(i)
                elif return_intermediates and i >= t_enc - 2:
                    intermediates.append(x_next)
                    inter_steps.append(i)
                if callback:
                    callback(i)
        out = {'x_encoded': x_next, 'intermediate_steps': inter_steps}
        if return_intermediates:
            out.update({'intermediates': intermediates})
        return x_next, out

    @staticmethod
    def _cat_cond(uc, c):
        """One 2B batch is possible when both branches carry the same hint tensors (guess_mode=False)."""
        if not (isinstance(uc, dict) and isinstance(c, dict)):
            return torch.cat([uc, c])
        hu, hc = uc.get('c_concat'), c.get('c_concat')
        if (hu is None) != (hc is None):
            return None
        if hu is not None:
            if len(hu) != len(hc) or any(a.data_ptr() != b.data_ptr() or a.shape != b.shape for a, b in zip(hu, hc)):
                return None
        if len(uc['c_crossattn']) != len(c['c_crossattn']):
            return None
        if any(a.shape[1:] != b.shape[1:] for a, b in zip(uc['c_crossattn'], c['c_crossattn'])):
            return None      # e.g. a 231-token prompt against a 77-token negative prompt: two calls (ddim_hacked.py:190-191)
        return {'c_concat': hc, 'c_crossattn': [torch.cat([a, b]) for a, b in zip(uc['c_crossattn'], c['c_crossattn'])]}

    def _batched_cond(self, uc, c):
        """A model whose UNet reads cat([x] + c_concat, 1) (LatentDiffusion with conditioning_key='hybrid') takes c_concat per
        ROW, unlike ControlLDM's hint: branches with different c_concat still make one 2B batch, with the parts concatenated
        along the batch like the contexts (the model then finds the halves unequal and drops its cfg_pairs shortcut).  Branches
        with the same c_concat keep the half-batch tensor of _cat_cond: one paired batch."""
        c_in = super()._batched_cond(uc, c)
        if c_in is None and getattr(getattr(getattr(self, 'model', None), 'model', None), 'conditioning_key', None) == 'hybrid' \
                and isinstance(uc, dict) and isinstance(c, dict):
            hu, hc, tu, tc = uc.get('c_concat'), c.get('c_concat'), uc['c_crossattn'], c['c_crossattn']
            if hu is not None and hc is not None and len(hu) == len(hc) and len(tu) == len(tc) \
                    and all(a.shape == b.shape for a, b in zip(hu, hc)) and all(a.shape[1:] == b.shape[1:] for a, b in zip(tu, tc)):
                c_in = {'c_concat': [torch.cat([a, b]) for a, b in zip(hu, hc)],
                        'c_crossattn': [torch.cat([a, b]) for a, b in zip(tu, tc)]}
                self._cin_memo = (*self._cin_memo[:2], c_in)        # the same joined tensors in every step, like the base memo's
        return c_in


# ----------------------------------------------------------------------------------------------- DPM-Solver++
class _DiscreteVPSchedule:
    """NoiseScheduleVP('discrete', alphas_cumprod=...) of ldm/models/diffusion/dpm_solver/dpm_solver.py:98-160:
    log alpha_t is the piecewise-linear interpolation of 0.5 log(alphas_cumprod) over t_k = k/N, k = 1..N (T = 1).
    Host-side float32 scalars, like the reference's float32 tensors."""

    def __init__(self, alphas_cumprod):
        ac = np.asarray(alphas_cumprod, dtype=np.float32)
        self.log_alpha = (np.float32(0.5) * np.log(ac)).astype(np.float32)
        self.total_N = len(ac)
        self.T = 1.0
        self.t_array = np.linspace(0., 1., self.total_N + 1, dtype=np.float32)[1:]

    def marginal_log_mean_coeff(self, t):
        """interpolate_fn (dpm_solver.py:1132-1171) for one scalar: linear between keypoints, linear extrapolation."""
        t = np.float32(t)
        xp, yp = self.t_array, self.log_alpha
        K = len(xp)
        idx = int(np.searchsorted(xp, t, side='left'))        # number of keypoints strictly below t
        if idx == 0:
            i0 = 0
        elif idx >= K:
            i0 = K - 2
        else:
            i0 = idx - 1
        x0, x1, y0, y1 = xp[i0], xp[i0 + 1], yp[i0], yp[i0 + 1]
        return np.float32(y0 + (t - x0) * (y1 - y0) / (x1 - x0))

    def marginal_alpha(self, t):
        return np.float32(np.exp(self.marginal_log_mean_coeff(t)))

    def marginal_std(self, t):
        return np.float32(np.sqrt(np.float32(1.) - np.exp(np.float32(2.) * self.marginal_log_mean_coeff(t))))

    def marginal_lambda(self, t):
        lm = self.marginal_log_mean_coeff(t)
        return np.float32(lm - np.float32(0.5) * np.log(np.float32(1.) - np.exp(np.float32(2.) * lm)))


DPMPP_FIRST, DPMPP_SECOND = 1, 2      # FGDM_DPMPP_FIRST / FGDM_DPMPP_SECOND of include/fgdm.h


def dpmpp_tables(ns, steps, order=2):
    """Every coefficient of a DPM-Solver++ multistep sampling (order 2, time_uniform, lower_order_final), one entry per network
    evaluation k = 0 .. steps - 1 at t_k, each followed by the update to t_{k+1}; float32 arithmetic, handed out as Python floats.
    The per-step route and the device loop (fgdm_sample_dpmpp) both read these tables, so they cannot drift apart.
      t_float                            the model's time input (t_k - 1/N) * 1000                        dpm_solver.py:278-287
      inv_alpha, neg_sigma_over_alpha    m0 = (x - sigma eps) / alpha as axpby(x, 1/alpha, eps, -sigma/alpha)         :386-399
      update_kind, c1, cm0, cm1          DPMPP_FIRST:  x = axpby(x, c1, m0, cm0)                                      :504-528
                                         DPMPP_SECOND: x = axpby(axpby(x, c1, m0, cm0), 1, m1, cm1)                   :755-789"""
    f32 = np.float32
    ts = np.linspace(ns.T, 1. / ns.total_N, steps + 1, dtype=np.float32)       # get_time_steps('time_uniform')
    tab = {k: [] for k in ('t_float', 'inv_alpha', 'neg_sigma_over_alpha', 'update_kind', 'c1', 'cm0', 'cm1')}
    for k in range(steps):
        s, t = ts[k], ts[k + 1]
        tab['t_float'].append(float((f32(s) - f32(1. / ns.total_N)) * f32(1000.)))
        a, sg = ns.marginal_alpha(s), ns.marginal_std(s)
        tab['inv_alpha'].append(float(f32(1.) / a))
        tab['neg_sigma_over_alpha'].append(float(-sg / a))
        step = k + 1                                                            # the reference's loop variable of this update
        step_order = 1 if k == 0 else (min(order, steps + 1 - step) if steps < 15 else order)      # init_order = 1; lower_order_final
        if step_order == 1:                                                     # dpm_solver.py:504-528 (predict_x0 branch)
            h = ns.marginal_lambda(t) - ns.marginal_lambda(s)
            c1 = ns.marginal_std(t) / ns.marginal_std(s)
            c2 = ns.marginal_alpha(t) * f32(np.expm1(-h))
            kind, cm0, cm1 = DPMPP_FIRST, float(-c2), 0.0
        else:                                                                   # dpm_solver.py:755-789 ('dpm_solver' type, predict_x0)
            t1, t0 = ts[k - 1], s
            l1, l0, lt = ns.marginal_lambda(t1), ns.marginal_lambda(t0), ns.marginal_lambda(t)
            h0, h = l0 - l1, lt - l0
            r0 = h0 / h
            c1 = ns.marginal_std(t) / ns.marginal_std(t0)
            c2 = ns.marginal_alpha(t) * (f32(np.exp(-h)) - f32(1.))
            # x_t = c1 x - c2 m0 - 0.5 c2 (m0 - m1) / r0
            kind, cm0, cm1 = DPMPP_SECOND, float(-c2 - f32(0.5) * c2 / r0), float(f32(0.5) * c2 / r0)
        tab['update_kind'].append(kind)
        tab['c1'].append(float(c1))
        tab['cm0'].append(cm0)
        tab['cm1'].append(cm1)
    return tab


class DPMSolverSampler:
    """ldm/models/diffusion/dpm_solver/sampler.py:8-82: DPM-Solver++ (data prediction), multistep order 2,
    time_uniform steps from T = 1 to 1/N, lower_order_final, classifier-free guidance as one 2B batch.
    The model is evaluated at FRACTIONAL timesteps (t - 1/N) * 1000 (dpm_solver.py:278-287).
    device_loop=True: the whole sampling is one engine call (fgdm_sample_dpmpp) when nothing asked for needs the host between
    steps, under the rule of the DDIM sampler's device loop; same tables (dpmpp_tables), same bits."""

    def __init__(self, model, device_loop=False, **kwargs):
        self.model = model
        self.device_loop = bool(device_loop)
        self.alphas_cumprod = torch.as_tensor(model.alphas_cumprod).clone().detach().to(torch.float32).to(model.device)

    def register_buffer(self, name, attr):
        setattr(self, name, attr)

    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None, img_callback=None,
               quantize_x0=False, eta=0., mask=None, x0=None, temperature=1., noise_dropout=0., score_corrector=None,
               corrector_kwargs=None, verbose=True, x_T=None, log_every_t=100, unconditional_guidance_scale=1.,
               unconditional_conditioning=None, **kwargs):
        if conditioning is not None:
            cbs = _SamplerBase._batch_of(conditioning)
            if cbs != batch_size:
                print(f"Warning: Got {cbs} conditionings but batch-size is {batch_size}")
        C, H, W = shape
        size = (batch_size, C, H, W)
        device = self.model.betas.device
        x = _randn(size, device) if x_T is None else x_T.to(device, torch.float32)
        ns = _DiscreteVPSchedule(self.alphas_cumprod.detach().cpu().numpy())
        steps, order = S, 2
        assert steps >= order
        scale, uc = unconditional_guidance_scale, unconditional_conditioning
        tab = dpmpp_tables(ns, steps, order)
        hooks = bool(callback or img_callback or score_corrector is not None or noise_dropout > 0.)
        plan = _loop_plan(self.model, self, conditioning, uc, [scale] * steps, None, None, x, hooks, kwargs, entry='sample_dpmpp')
        if plan is not None:            # (mask / x0 are ignored, as the reference's sampler ignores them)
            ctx, uctx, flags, control_scales = plan
            x = self.model.engine.sample_dpmpp(x, ctx, uctx, scale if uctx is not None else 1.0, tab,
                                               control_scales=control_scales, flags=flags)
            return x.to(device), None

        def data_prediction(xx, k):
            # model_wrapper (classifier-free, dpm_solver.py:321-343) + data_prediction_fn (:386-399) of evaluation k
            t_in = torch.full((xx.shape[0],), tab['t_float'][k], device=xx.device, dtype=torch.float32)
            if scale == 1. or uc is None:
                e = self.model.apply_model(xx, t_in, conditioning)
            else:
                kw = {'cfg_pairs': True} if getattr(self.model, 'engine', None) is not None else {}
                out = self.model.apply_model(torch.cat([xx] * 2), torch.cat([t_in] * 2), torch.cat([uc, conditioning]), **kw)
                e_u, e_c = out.chunk(2)
                e = _k.cfg_combine(e_c.contiguous(), e_u.contiguous(), scale)
            return _k.axpby(xx.contiguous(), tab['inv_alpha'][k], e, tab['neg_sigma_over_alpha'][k])     # (x - sigma eps) / alpha

        def update(xx, k, m0, m1):       # from t_k to t_{k+1} behind evaluation k: first_update / second_update (dpm_solver.py:504-528, 755-789)
            y = _k.axpby(xx, tab['c1'][k], m0, tab['cm0'][k])
            return y if tab['update_kind'][k] == DPMPP_FIRST else _k.axpby(y, 1.0, m1, tab['cm1'][k])

        m_prev = [data_prediction(x, 0)]
        x = update(x, 0, m_prev[-1], None)                      # init_order = 1
        m_prev.append(data_prediction(x, 1))
        for step in range(order, steps + 1):
            x = update(x, step - 1, m_prev[1], m_prev[0])
            m_prev = [m_prev[1], m_prev[1]]
            if step < steps:
                m_prev[-1] = data_prediction(x, step)
            if callback:
                callback(step)
        return x.to(device), None
