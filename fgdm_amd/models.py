"""Host-side mirrors of the reference's model objects for the sampling path.

  LatentDiffusion  <-  ldm/models/diffusion/ddpm.py  (register_schedule :175-227, apply_model :1035-1136,
                       q_sample :342-345, predict_start_from_noise :284-288, q_posterior :290-297,
                       p_mean_variance :1260-1292, p_sample :1295-1323, p_sample_loop :1382-1430, sample :1433-1448)
  ControlLDM       <-  controlnet/cldm/cldm.py:816-849 (apply_model with dict conds, control_scales)

They expose what the samplers and the inference scripts require of `model`: num_timesteps, betas,
alphas_cumprod(_prev), device, parameterization, apply_model, q_sample, control_scales, cuda()/to()/eval(),
ema_scope(), load_state_dict().  All network arithmetic runs in the HIP engine; the per-step latent updates run
in the sampler kernels.  decode_first_stage (ddpm.py:832-889) runs in the engine too when the
model is built with a `first_stage_config` -- and encode_first_stage / get_first_stage_encoding (ddpm.py:952-996, 648-661)
when it is also built with `first_stage_encoder=True` -- and get_learned_conditioning (FrozenCLIPEmbedder's transformer,
ldm/modules/encoders/modules.py:137-162) when it is built with a `cond_stage_config`; only the BPE
tokenizer (host code of the third-party `transformers` package) stays outside: `model.tokenizer`.
"""
import contextlib

import numpy as np
import torch

from . import _lib, config as _cfg, hack as _hack, patches as _patches, schedule
from . import engine as _k


def _randn(shape, device):
    return torch.randn(shape, device=device)


def plan_noise_segments(steps, step_bytes, max_bytes):
    """The device ancestral loop's walk of `steps` steps, each needing step_bytes of pre-drawn noise, as consecutive segments
    [(start, stop), ...] of at most max_bytes of noise each: as many whole steps as fit, one step where a single step already
    exceeds the bound.  The segments cover range(steps) once and in order; a pure function."""
    per = max(1, int(max_bytes) // max(1, int(step_bytes)))
    return [(a, min(a + per, steps)) for a in range(0, steps, per)]


class _Buffers:
    """schedule tables as float32 torch tensors on the model's device (attribute names of register_schedule)."""

    def _register_schedule(self, device, **kw):
        tabs = schedule.ddpm_tables(**kw)
        for k, v in tabs.items():
            setattr(self, k, torch.from_numpy(v).to(device))
        self._host = tabs
        self.num_timesteps = int(tabs['betas'].shape[0])


class DiagonalGaussianDistribution:
    """ldm/modules/distributions/distributions.py:24-63: the posterior AutoencoderKL.encode returns.  `parameters` holds
    mean | log-variance along dim 1.  On the GPU sample() and mode() are one launch of the engine's posterior kernel; the
    remaining members (std, var, kl, nll: training-side quantities) are plain tensor expressions, as are all of them on CPU tensors."""

    def __init__(self, parameters, deterministic=False):
        self.parameters = parameters
        self.mean, logvar = torch.chunk(parameters, 2, dim=1)
        self.logvar = torch.clamp(logvar, -30.0, 20.0)
        self.deterministic = deterministic
        if deterministic:
            self.var = self.std = torch.zeros_like(self.mean)
        else:
            self.std = torch.exp(0.5 * self.logvar)
            self.var = torch.exp(self.logvar)

    def sample(self, scale=1.0):
        """mean + std * noise; the noise is drawn on the CPU generator and moved to the device, as the reference draws it
        (distributions.py:36), so one torch.manual_seed gives both the same noise.  `scale` (not in the reference) folds the
        scale_factor of get_first_stage_encoding into the same kernel."""
        noise = torch.randn(self.mean.shape).to(device=self.parameters.device)
        if self.parameters.is_cuda and not self.deterministic:
            return _k.posterior_sample(self.parameters, noise, scale)
        x = self.mean + self.std * noise
        return x if scale == 1.0 else scale * x

    def mode(self, scale=1.0):
        if self.parameters.is_cuda:
            return _k.posterior_sample(self.parameters, None, scale)
        return self.mean if scale == 1.0 else scale * self.mean

    def kl(self, other=None):
        if self.deterministic:
            return torch.Tensor([0.])
        if other is None:
            return 0.5 * torch.sum(self.mean ** 2 + self.var - 1.0 - self.logvar, dim=[1, 2, 3])
        return 0.5 * torch.sum((self.mean - other.mean) ** 2 / other.var + self.var / other.var - 1.0 - self.logvar + other.logvar,
                               dim=[1, 2, 3])

    def nll(self, sample, dims=(1, 2, 3)):
        if self.deterministic:
            return torch.Tensor([0.])
        return 0.5 * torch.sum(float(np.log(2.0 * np.pi)) + self.logvar + (sample - self.mean) ** 2 / self.var, dim=list(dims))


class DiffusionWrapper:
    """ddpm.py:1829-1848: holds `.diffusion_model` (here: the HIP engine) and the conditioning key."""

    def __init__(self, engine, conditioning_key):
        self.diffusion_model = engine
        self.conditioning_key = conditioning_key


# DiffusionWrapper.forward's modes (ddpm.py:1829-1846) the engine has no network for, each with its reason
_REFUSED_KEYS = {
    'concat': "conditioning_key='concat' hands the UNet cat([x] + c_concat, 1) WITHOUT a context (ddpm.py:1832-1834): the engine "
              "builds UNets whose SpatialTransformers take a text context; use 'hybrid' (c_concat and c_crossattn)",
    'adm': "conditioning_key='adm' hands the UNet class embeddings, y=c_crossattn[0] (ddpm.py:1842-1844): the engine has no "
           'label embedding (num_classes is fixed to None)',
    None: 'conditioning_key=None is the unconditional UNet (ddpm.py:1830-1831): the engine builds UNets whose SpatialTransformers '
          'take a text context',
}


class LatentDiffusion(_Buffers):
    def __init__(self, unet_config=None, engine=None, use_adapter=None, n_controlnets=0, num_prompts=1, timesteps=1000,
                 beta_schedule='linear', linear_start=0.00085, linear_end=0.012, cosine_s=8e-3, given_betas=None,
                 v_posterior=0.0, parameterization='eps', conditioning_key='crossattn', scale_factor=0.18215,
                 channels=4, image_size=32, log_every_t=200, clip_denoised=False, device=0, first_stage_config=None,
                 cond_stage_config=None, first_stage_encoder=False, device_loop=False, device_noise=None, **ignored):
        if parameterization != 'eps':
            raise NotImplementedError(f'parameterization={parameterization!r}: only eps-parameterization is implemented (the shipped '
                                      f'configs, models/config.yaml; {_cfg.SD2_LIMIT}; v-prediction checkpoints are refused)')
        if conditioning_key not in ('crossattn', 'hybrid'):
            raise NotImplementedError(_REFUSED_KEYS.get(conditioning_key, f'conditioning_key={conditioning_key!r}: DiffusionWrapper '
                                                                          "knows None, 'concat', 'crossattn', 'hybrid', 'adm'"))
        self.engine = engine if engine is not None else _k.Engine(device=device, **self.engine_args(
            unet_config=unet_config, use_adapter=use_adapter, n_controlnets=n_controlnets, num_prompts=num_prompts,
            first_stage_config=first_stage_config, cond_stage_config=cond_stage_config, first_stage_encoder=first_stage_encoder))
        self.device = self.engine.device
        self.model = DiffusionWrapper(self.engine, conditioning_key)
        self.parameterization = parameterization
        self.v_posterior = v_posterior
        self.scale_factor = scale_factor
        self.channels = channels
        self.image_size = image_size
        self.log_every_t = log_every_t
        self.clip_denoised = clip_denoised
        self.shorten_cond_schedule = False
        self.cond_stage_model = None        # optional callable(list[str]) -> [B,77,768] overriding the engine's text encoder
        self.tokenizer = None               # callable(list[str]) -> int64 ids [B,77]; default: transformers.CLIPTokenizer
        self.clip_version = 'openai/clip-vit-large-patch14'
        self.max_length = 77
        self.raw_tokenizer = None           # callable(list[str]) -> list[list[int]] without special tokens (the long-prompt route)
        self.special_tokens = None          # (BOS, EOS, PAD) of raw_tokenizer; default: the tokenizer's own, else CLIP's
        self.clip_hack, self.clip_skip = _hack.state()      # controlnet/cldm/hack.py:23-28 (hack_everything)
        self.first_stage_decode = None      # optional callable(z / scale_factor) -> image overriding the engine's decoder
        self.first_stage_encode = None      # optional callable(image) -> posterior (or latent tensor) overriding the engine's encoder
        self._register_schedule(self.device, kind=beta_schedule, timesteps=timesteps, linear_start=linear_start,
                                linear_end=linear_end, cosine_s=cosine_s, v_posterior=v_posterior,
                                given_betas=given_betas)
        self._finalized = False
        self.device_loop = bool(device_loop)                # p_sample_loop / sample as engine calls where nothing needs the host between steps
        self.max_loop_noise_bytes = 256 << 20               # pre-drawn noise per engine call of that route: a memory bound, not a tuned number
        # None: p_sample / q_sample draw from torch's generator.  A seed: from the engine's counter-based generator (fgdm_loop_noise_set /
        # fgdm_randn, include/fgdm.h) -- the device route then draws nothing on the host, holds no noise planes and runs the whole walk
        # as ONE engine call; the per-step route takes the same numbers from Engine.randn, so both still agree bit for bit.  x_T stays
        # a torch draw.  noise_first_sample: the global index of row 0 (a rank's shard offset, fgdm_amd.dist).
        self.device_noise = device_noise
        self.noise_first_sample = 0
        self._noise_pos = 0                                 # walk position of the step the per-step route is in

    def _generated(self, stream, shape, repeat=False):
        """the per-step route's draw at the walk position it is in, from the engine's generator (device_noise is a seed)"""
        return _k.randn(self.device_noise, stream, self._noise_pos, shape, self.noise_first_sample, repeat, device=self.device)

    @classmethod
    def engine_args(cls, unet_config=None, use_adapter=None, n_controlnets=0, num_prompts=1, first_stage_config=None,
                    cond_stage_config=None, first_stage_encoder=False, **ignored):
        """Constructor arguments of the reference model -> keyword arguments of fgdm_amd.engine.Engine / make_config (a pure
        function: works without a GPU).  unet_config as the scripts pass it: {target: ...UNetModel, params: {...}}
        (models/config.yaml:33-48; OmegaConf or dict) or the bare parameter dict; the target and its flags select the
        adapter variant the engine builds."""
        kind, cfg, uflags = _cfg.unet_params(unet_config)
        asked = bool(use_adapter)                     # the caller's own request; None: the FG-DM default, an adapter
        use_adapter = True if use_adapter is None else use_adapter
        if kind == 'controlled' or uflags.get('no_prompting'):
            use_adapter = False                       # ControlledUnetModel / no_prompting: the plain SD UNet
        elif uflags.get('use_time_adapter'):
            use_adapter = 'time'
        if cfg is not None and cfg['in_channels'] != 4 and use_adapter:
            # a UNet fed cat([x] + c_concat, 1) ('hybrid'): UNetModel.forward would hand that input to an adapter built for 4
            # channels (openaimodel.py:836-844), so such networks are the plain SD UNet apart from conv_in
            if asked or uflags.get('use_time_adapter'):
                raise NotImplementedError(f"in_channels={cfg['in_channels']} with an FG-DM adapter: the adapter takes the 4 latent "
                                          'channels, the reference hands it the concatenated input (openaimodel.py:836-844)')
            use_adapter = False
        if kind == 'adapt' or uflags.get('num_prompts', 1) > 1:
            num_prompts = max(num_prompts, int(uflags.get('num_prompts', num_prompts)))
        args = dict(cfg=cfg, use_adapter=use_adapter, n_controlnets=n_controlnets, num_prompts=num_prompts,
                    vae=cls._ddconfig(first_stage_config), clip=cls._clipconfig(cond_stage_config))
        if first_stage_encoder:       # (absent otherwise: models built as before ask the engine for what they asked before)
            args['vae_encoder'] = True
        return args

    @staticmethod
    def _ddconfig(first_stage_config):
        """first_stage_config as in models/config.yaml:50-71 ({'target': ..., 'params': {'ddconfig': {...}}}), a bare
        ddconfig dict, True (SD-v1 decoder) or None (no decoder in the engine)."""
        if not first_stage_config:
            return None
        if first_stage_config is True:
            return True
        fc = dict(first_stage_config)
        if 'params' in fc:
            fc = dict(fc['params'])
        return dict(fc.get('ddconfig', fc))

    @staticmethod
    def _clipconfig(cond_stage_config):
        """cond_stage_config as in models/config.yaml:73-74 ({'target': '...FrozenCLIPEmbedder'}), True (SD-v1 text tower),
        a CLIPTextConfig-style dict, or None (no text encoder in the engine)."""
        if not cond_stage_config:
            return None
        if cond_stage_config is True:
            return True
        cc = dict(cond_stage_config)
        if 'target' in cc:
            if 'OpenCLIP' in str(cc['target']):
                raise NotImplementedError(f"cond_stage_config target {cc['target']}: the OpenCLIP text encoder is not in the engine; "
                                          f'{_cfg.SD2_LIMIT} (build the model without cond_stage_config and set its '
                                          'cond_stage_model, or pass c_crossattn tensors [B, tokens, 1024])')
            if not str(cc['target']).endswith('FrozenCLIPEmbedder'):
                raise NotImplementedError(f"cond_stage_config target {cc['target']}: only FrozenCLIPEmbedder is shipped")
            return True
        return cc

    # ---- nn.Module-ish surface the scripts touch (scripts/txt2img_fgdm_inference.py:23-38,179-180,216-218)
    def cuda(self, *a, **k):
        return self

    def cpu(self, *a, **k):          # create_model(...).cpu() (controlnet/cldm/model.py:26): the engine lives on its GPU
        return self

    def to(self, *a, **k):
        return self

    def eval(self):
        return self

    @contextlib.contextmanager
    def ema_scope(self, context=None):
        yield None          # use_ema: False in every shipped config

    def load_state_dict(self, sd, strict=False):
        missing = self.engine.load_state_dict(sd, strict=strict)
        want = self.engine.param_shapes()
        unexpected = [k for k in sd if k not in want]
        if not missing:
            self.engine.finalize()
            self._finalized = True
        return missing, unexpected

    def load_lora(self, lora_state_dict, base_state_dict, scale=1.0):
        """Merge a LoRA adapter (fgdm_amd/lora.py: ldm or kohya key names) into the finalized engine in place: the UNet, the
        ControlNets (`control_model.` keys) and the text tower when the engine has one.  base_state_dict: the checkpoint the engine
        was loaded from (the packed engine keeps no fp32 weights).  A further call merges on top: the sum is rebuilt from the base
        with the deltas in call order.  The effective scale of a module is scale * alpha / rank."""
        from . import lora
        self._loras = lora.load(self.engine, getattr(self, '_loras', []), lora_state_dict, base_state_dict, scale)

    def unload_lora(self):
        """Put back, byte for byte, the packed weights from before the first load_lora."""
        if getattr(self, '_loras', None):
            self.engine.weights_restore()
            self._loras = []

    def _tokenize(self, text):
        """FrozenCLIPEmbedder.forward's tokenizer call (modules.py:153-155)."""
        if self.tokenizer is None:
            try:
                from transformers import CLIPTokenizer
                tok = CLIPTokenizer.from_pretrained(self.clip_version)
            except Exception as e:      # no vocabulary files on this machine (no network)
                raise RuntimeError(f'CLIP tokenizer files for {self.clip_version} are not available ({e}); set '
                                   'model.tokenizer to a callable list[str] -> int64 ids [B, 77]') from e
            self.tokenizer = lambda t: tok(t, truncation=True, max_length=self.max_length, return_length=True,
                                           return_overflowing_tokens=False, padding='max_length',
                                           return_tensors='pt')['input_ids']
        return self.tokenizer(text)

    def _tokenize_raw(self, text):
        """_hacked_clip_forward's tokenizer call (controlnet/cldm/hack.py:33-38): raw ids, no special tokens, no truncation."""
        if self.raw_tokenizer is None:
            try:
                from transformers import CLIPTokenizer
                tok = CLIPTokenizer.from_pretrained(self.clip_version)
            except Exception as e:      # no vocabulary files on this machine (no network)
                raise RuntimeError(f'CLIP tokenizer files for {self.clip_version} are not available ({e}); set '
                                   'model.raw_tokenizer to a callable list[str] -> list[list[int]] (no special tokens)') from e
            self.raw_tokenizer = lambda t: tok(t, truncation=False, add_special_tokens=False)['input_ids']
            if self.special_tokens is None:
                self.special_tokens = (tok.bos_token_id, tok.eos_token_id, tok.pad_token_id)
        return self.raw_tokenizer(text)

    def get_learned_conditioning(self, c):
        """ddpm.py get_learned_conditioning -> cond_stage_model.encode(c): list of prompts (or ready token ids) ->
        [B, 77, 768]; after hack_everything (controlnet/cldm/hack.py:23-68) three 75-token chunks per prompt -> [B, 231, 768],
        and ready token ids are then read as [B, 3, 77] (or [3B, 77]) chunk arrays."""
        if self.cond_stage_model is not None:
            return self.cond_stage_model(c)
        if not getattr(self.engine, 'has_clip', False):
            raise NotImplementedError('this model was built without cond_stage_config; pass one (or set '
                                      'model.cond_stage_model to a callable returning [B,77,768])')
        ready = torch.is_tensor(c) or isinstance(c, np.ndarray)
        if self.clip_hack:
            if ready:
                ids = torch.as_tensor(c).reshape(-1, _hack.MAX_LENGTH)
                y = self.engine.clip_encode(ids, clip_skip=self.clip_skip)
                return y.reshape(-1, _hack.CHUNKS * _hack.MAX_LENGTH, y.shape[-1])
            raw = self._tokenize_raw(list(c))
            bos, eos, pad = self.special_tokens or (_hack.BOS, _hack.EOS, _hack.PAD)
            return _hack.encode(self.engine, raw, self.clip_skip, bos, eos, pad)
        ids = c if ready else self._tokenize(list(c))
        return self.engine.clip_encode(ids)

    def decode_first_stage(self, z, predict_cids=False, force_not_quantize=False, n=None):
        """ddpm.py:832-889 for an AutoencoderKL first stage: decode(z / scale_factor).  A model carrying `split_input_params`
        with patch_distributed_vq decodes overlapping latent crops and blends them (ddpm.py:841-878); a non-square crop or a
        grid the crops do not cover is a ValueError (fgdm_amd/patches.py)."""
        if predict_cids:
            raise NotImplementedError('predict_cids needs a VQ first stage; every shipped config uses AutoencoderKL')
        sp = getattr(self, 'split_input_params', None)
        if sp is not None and sp['patch_distributed_vq']:
            return self._decode_patches(z, sp)
        if self.first_stage_decode is not None:
            return self.first_stage_decode(1. / self.scale_factor * z)
        if not self.engine.has_vae:
            raise NotImplementedError('this model was built without first_stage_config; pass one (or set '
                                      'model.first_stage_decode to a callable)')
        return self.engine.vae_decode(z, 1. / self.scale_factor)

    def _patch_tables(self, kh, kw, Ly, Lx, sp):
        """(w_pix, w_tie) on the model's device, computed once per geometry and clipping parameters"""
        key = (kh, kw, Ly, Lx, bool(sp.get('tie_braker', False)), sp['clip_min_weight'], sp['clip_max_weight'],
               sp.get('clip_min_tie_weight'), sp.get('clip_max_tie_weight'))
        memo = self.__dict__.setdefault('_patch_tables_memo', {})
        if key not in memo:
            memo[key] = tuple(v.to(self.device) for v in _patches.weights(kh, kw, Ly, Lx, sp))
        return memo[key]

    def _decode_patches(self, z, sp):
        (kh, kw), stride, Ly, Lx, f = _patches.decode_geometry(z.shape[2], z.shape[3], sp)
        w_pix, w_tie = self._patch_tables(kh * f, kw * f, Ly, Lx, sp)
        if self.first_stage_decode is not None:      # a caller's own decoder: its crops through the engine's unfold / fold
            crops = _k.unfold((1. / self.scale_factor * z).to(self.device), (kh, kw), stride)
            o = torch.stack([self.first_stage_decode(c) for c in crops])
            return _k.fold_weighted(o, w_pix, w_tie, (z.shape[2] * f, z.shape[3] * f), (stride[0] * f, stride[1] * f))
        if not self.engine.has_vae:
            raise NotImplementedError('this model was built without first_stage_config; pass one (or set '
                                      'model.first_stage_decode to a callable)')
        return self.engine.vae_decode_patches(z, 1. / self.scale_factor, (kh, kw), stride, f, w_pix, w_tie,
                                              getattr(self, 'max_crops_per_pass', 0))

    def encode_first_stage(self, x):
        """ddpm.py:952-996 for an AutoencoderKL first stage (plain branch): first_stage_model.encode(x), the posterior of an
        image batch fp32 NCHW [B,3,H,W] in [-1,1]."""
        if hasattr(self, 'split_input_params'):
            raise NotImplementedError('split_input_params: patch-wise encoding cannot run with an AutoencoderKL first stage -- the '
                                      "reference's branch (ddpm.py:957-984) multiplies the DiagonalGaussianDistribution that "
                                      'encode() returns by the weighting tensor')
        if self.first_stage_encode is not None:
            return self.first_stage_encode(x)
        if not getattr(self.engine, 'has_vae_encoder', False):
            raise NotImplementedError('this model was built without the first-stage encoder; build it with first_stage_config '
                                      'and first_stage_encoder=True (Engine(..., vae=..., vae_encoder=True)), or set '
                                      'model.first_stage_encode to a callable')
        return DiagonalGaussianDistribution(self.engine.vae_encode(x))

    def get_first_stage_encoding(self, encoder_posterior):
        """ddpm.py:648-661: scale_factor * (a sample of the posterior | the tensor itself | the channel concat of samples)."""
        if isinstance(encoder_posterior, list):
            return torch.cat([item.sample(self.scale_factor) if isinstance(item, DiagonalGaussianDistribution)
                              else self.scale_factor * item.sample() for item in encoder_posterior], 1)
        if isinstance(encoder_posterior, DiagonalGaussianDistribution):
            return encoder_posterior.sample(self.scale_factor)
        if isinstance(encoder_posterior, torch.Tensor):
            if encoder_posterior.is_cuda and encoder_posterior.dtype == torch.float32:
                return _k.axpby(encoder_posterior.contiguous(), self.scale_factor, None, 0.0)
            return self.scale_factor * encoder_posterior
        raise NotImplementedError(f"encoder_posterior of type '{type(encoder_posterior)}' not yet implemented")

    # ---- apply_model (ddpm.py:1035-1044,1130-1136 non-tiled branch; DiffusionWrapper crossattn mode)
    def _context(self, cond):
        """cc = torch.cat(c_crossattn, 1) (ddpm.py:1835-1837; cldm.py:846).  Several parts are joined once per list of tensor
        objects: the samplers pass the same parts in every step, and handing the engine the SAME joined tensor lets it keep
        the context's K/V projections.  The memo holds the parts, so their ids cannot be recycled (_version: in-place writes)."""
        if isinstance(cond, dict):
            cc = cond['c_crossattn']
        elif isinstance(cond, (list, tuple)):
            cc = list(cond)
        else:
            cc = [cond]
        if len(cc) == 1:
            return cc[0]
        key = tuple((id(t), t._version) for t in cc)
        memo = getattr(self, '_ctx_cat_memo', None)
        if memo is None or memo[0] != key:
            self._ctx_cat_memo = memo = (key, list(cc), torch.cat(cc, 1))
        return memo[2]

    def _apply_model_patches(self, x_noisy, t, cond, return_ids, sp):
        """ddpm.py:1046-1128, text-conditioning branch: the UNet on every crop with the same t and cond, blended.  As in the
        reference, **kwargs of apply_model (pcond, use_original, cfg_pairs, conds) are not forwarded to the crops (:1119)."""
        ncond = len(cond) if isinstance(cond, dict) else 1       # a tensor or a list becomes {'c_crossattn': cond} (:1037-1044)
        assert ncond == 1      # todo of the reference: can only deal with one conditioning
        assert not return_ids
        if getattr(self, 'cond_stage_key', None) in _patches.SPATIAL_COND_KEYS:
            raise NotImplementedError(f"split_input_params with cond_stage_key '{self.cond_stage_key}' (a conditioning that is cut "
                                      'into crops, or crop coordinates) is not supported: only the text branch is')
        if getattr(self.engine, 'n_controlnets', 0):
            raise NotImplementedError('split_input_params: ControlLDM.apply_model has no patch branch in the reference')
        (kh, kw), stride, Ly, Lx = _patches.plan(x_noisy.shape[2], x_noisy.shape[3], sp['ks'], sp['stride'], clamp=False)
        w_pix, w_tie = self._patch_tables(kh, kw, Ly, Lx, sp)
        return self.engine.apply_model_patches(x_noisy, t, self._context(cond), (kh, kw), stride, w_pix, w_tie,
                                               getattr(self, 'max_crops_per_pass', 0))

    def _concat(self, x_noisy, cond):
        """xc = torch.cat([x] + c_concat, dim=1) (ddpm.py:1838-1841), the c_concat side: the channel-wise join of the parts, made
        once per list of tensor objects (and _version) like _context's, so that the engine sees the SAME tensor in every step and
        keeps its stored copy.  -> (joined tensor, may_pair): its rows are the batch, or half of it (a sampler's cat([x] * 2)
        batch sharing one image); may_pair tells whether rows b and b + B/2 of the batch read equal c_concat rows."""
        if not isinstance(cond, dict):
            raise TypeError("conditioning_key='hybrid' needs a dict cond {'c_concat': [...], 'c_crossattn': [...]} (the reference "
                            f'fails on [x] + None, ddpm.py:1840); got {type(cond).__name__}')
        parts = cond.get('c_concat')
        if not isinstance(parts, (list, tuple)) or not parts or 'c_crossattn' not in cond:
            raise TypeError("conditioning_key='hybrid' needs cond['c_concat'] (a list of tensors) and cond['c_crossattn']")
        if len(parts) == 1:
            cc = parts[0]
        else:
            key = tuple((id(p), p._version) for p in parts)
            memo = getattr(self, '_concat_cat_memo', None)
            if memo is None or memo[0] != key:
                self._concat_cat_memo = memo = (key, list(parts), torch.cat(list(parts), 1))
            cc = memo[2]
        B = x_noisy.shape[0]
        if cc.dim() != 4 or tuple(cc.shape[2:]) != tuple(x_noisy.shape[2:]) or not (cc.shape[0] == B or 2 * cc.shape[0] == B):
            raise ValueError(f'c_concat {tuple(cc.shape)} does not fit the latent batch {tuple(x_noisy.shape)}')
        return cc, (2 * cc.shape[0] == B or self._halves_equal(cc))

    def capture_attention(self, blocks=None, tokens=None, rows='cond', mode='sum', latent=None, **kw):
        """Engine.capture_attention with blocks named by place and resolution, as ptp_utils users select them: 'down', 'mid', 'up',
        ('up', 16), or a side of the map alone -- here an int IS a side (16: the 16 x 16 blocks of a latent of image_size cells;
        block indices go to Engine.capture_attention)."""
        if blocks is not None:
            blocks = [blocks] if isinstance(blocks, (str, int)) or (isinstance(blocks, tuple) and isinstance(blocks[0], str)) else list(blocks)
            blocks = [str(b) if isinstance(b, int) and not isinstance(b, bool) else b for b in blocks]
        return self.engine.capture_attention(blocks=blocks, tokens=tokens, rows=rows, mode=mode,
                                             latent=self.image_size if latent is None else latent, **kw)

    def apply_model(self, x_noisy, t, cond, return_ids=False, **kwargs):
        sp = getattr(self, 'split_input_params', None)
        hybrid = self.model.conditioning_key == 'hybrid'
        if hybrid and sp is not None:
            raise NotImplementedError("split_input_params with conditioning_key='hybrid': the reference's patch branch crops c_concat "
                                      'only for its spatial cond_stage_keys (ddpm.py:1061-1071), which are not supported')
        if sp is not None:
            return self._apply_model_patches(x_noisy, t, cond, return_ids, sp)
        if return_ids:
            raise NotImplementedError('return_ids / return_conds needs a model with two outputs; no shipped model has one')
        if hybrid:
            cc, may_pair = self._concat(x_noisy, cond)
            self.engine.set_concat(cc)                # a no-op while the same tensor is handed over
            flags = _lib.FLAG_NO_CONTROL | (_lib.FLAG_USE_ORIGINAL if kwargs.get('use_original', False) else 0)
            # cfg_pairs (set by the samplers for cat([x] * 2) batches): honoured only if both halves read the same c_concat rows
            if kwargs.get('cfg_pairs', False) and may_pair:
                flags |= _lib.FLAG_CFG_PAIRS
            return self.engine.apply_model(x_noisy, t, self._context(cond), flags=flags)
        flags = _lib.FLAG_NO_CONTROL
        if kwargs.get('use_original', False):
            flags |= _lib.FLAG_USE_ORIGINAL
        # AdaptUNetModel.forward(x, t, context, control=None, conds=None) (openaimodel.py:1263): `control` replaces the
        # adapter's prompt (UNetModel calls it `pcond`), `conds` feed the extra adapters
        if 'conds' in kwargs or getattr(self.engine, '_conds_key', None) is not None:
            self.engine.set_adapter_conds(kwargs.get('conds'))
        pcond = kwargs.get('pcond', kwargs.get('control'))
        # cfg_pairs (set by the samplers for cat([x] * 2) batches): the engine evaluates the network prefix on the first
        # half only, which is exact only if the two halves of a user-supplied prompt image are the same rows too
        if kwargs.get('cfg_pairs', False) and (pcond is None or self._halves_equal(pcond)):
            flags |= _lib.FLAG_CFG_PAIRS
        return self.engine.apply_model(x_noisy, t, self._context(cond), flags=flags, pcond=pcond)

    def _halves_equal(self, v):
        """True iff v[:B/2] == v[B/2:] (checked once per tensor object / version: the samplers pass the same object every
        step).  The memo keeps the tensor alive so its id cannot be recycled."""
        key = (id(v), v._version, tuple(v.shape))
        memo = getattr(self, '_halves_memo', None)
        if memo is None or memo[0] != key:
            n = v.shape[0]
            eq = n % 2 == 0 and bool(torch.equal(v[:n // 2], v[n // 2:]))
            self._halves_memo = memo = (key, v, eq)
        return memo[2]

    # ---- closed-form pieces
    def _at(self, name, t):
        return [float(v) for v in self._host[name][np.asarray(t.detach().cpu())]]

    def q_sample(self, x_start, t, noise=None):
        """sqrt(acp_t) x0 + sqrt(1-acp_t) noise; per-sample t handled by grouping equal timesteps."""
        noise = torch.randn_like(x_start) if noise is None else noise
        a, b = self._at('sqrt_alphas_cumprod', t), self._at('sqrt_one_minus_alphas_cumprod', t)
        if len(set(a)) == 1:
            return _k.axpby(x_start.contiguous(), a[0], noise.contiguous(), b[0])
        return torch.cat([_k.axpby(x_start[i:i + 1].contiguous(), a[i], noise[i:i + 1].contiguous(), b[i])
                          for i in range(x_start.shape[0])])

    def predict_start_from_noise(self, x_t, t, noise):
        a, b = self._at('sqrt_recip_alphas_cumprod', t), self._at('sqrt_recipm1_alphas_cumprod', t)
        assert len(set(a)) == 1, 'per-sample timesteps: call per sample'
        return _k.axpby(x_t.contiguous(), a[0], noise.contiguous(), -b[0])

    def p_sample(self, x, c, t, clip_denoised=False, repeat_noise=False, return_x0=False, temperature=1.,
                 noise_dropout=0., noise=None, **kwargs):
        """One ancestral step; all samples of a call share t (as in p_sample_loop, ddpm.py:1407)."""
        if clip_denoised or noise_dropout > 0.:
            raise NotImplementedError('clip_denoised / noise_dropout are not used by the latent configs')
        ti = int(t[0])
        assert bool((t == ti).all()), 'p_sample expects one timestep per call'
        eps = self.apply_model(x, t, c, **kwargs)
        h = self._host
        if noise is None and getattr(self, 'device_noise', None) is not None:
            noise = self._generated(_lib.NOISE_STREAM_STEP, x.shape, repeat_noise)
        elif noise is None:
            noise = _randn((1, *x.shape[1:]) if repeat_noise else x.shape, x.device)
            noise = noise.expand_as(x).contiguous()
        std = 0.0 if ti == 0 else float(np.exp(0.5 * h['posterior_log_variance_clipped'][ti])) * temperature
        out = _k.ancestral_step(x.contiguous(), eps, h['sqrt_recip_alphas_cumprod'][ti],
                                h['sqrt_recipm1_alphas_cumprod'][ti], h['posterior_mean_coef1'][ti],
                                h['posterior_mean_coef2'][ti], std, noise if ti != 0 else None)
        if return_x0:
            return out, self.predict_start_from_noise(x, t, eps)
        return out

    # ---- the device ancestral loop (fgdm_sample_ancestral)
    def _ancestral_plan(self, cond, img, timesteps, mask, x0, host_hooks, kwargs):
        """None (per-step route), or (ctx, None, flags, control_scales) for the device loop: the rule the samplers' _loop_plan
        applies -- nothing asked for runs on the host between steps, and a conditioning the engine's loops take.  Draws no noise."""
        from . import samplers
        eng = self.engine
        if not getattr(self, 'device_loop', False) or host_hooks or timesteps < 1 or not hasattr(eng, 'sample_ancestral'):
            return None
        if set(kwargs) - {'repeat_noise', 'temperature'} or self.clip_denoised:
            return None                 # return_x0, a caller's noise, apply_model's keywords, the refused options: p_sample's business
        if getattr(self, 'split_input_params', None) is not None or img.dim() != 4 or img.shape[1] != 4:
            return None
        if mask is not None and (x0 is None or tuple(x0.shape) != tuple(img.shape)):
            return None
        if not isinstance(self, ControlLDM):        # {'c_crossattn': [ctx]} and [ctx] are the tensor ctx (apply_model's _context)
            if isinstance(cond, dict) and cond.get('c_concat') is None:
                cond = cond.get('c_crossattn')
            if isinstance(cond, (list, tuple)) and len(cond) == 1:
                cond = cond[0]
        return samplers._loop_cond(self, cond, None, False)

    def _device_ancestral(self, plan, img, timesteps, mask, x0, log_every_t, repeat_noise=False, temperature=1.):
        """The walk t = timesteps - 1 ... 0 as consecutive engine calls of at most max_loop_noise_bytes of pre-drawn noise each.
        The noise is drawn by the calls of the per-step route in its order -- per step p_sample's, then q_sample's if there is a
        mask -- so the same generator state gives the same bits.  log_every_t None: nothing is logged.  -> (img, the logged latents)."""
        ctx, _, flags, control_scales = plan
        h = self._host
        ts = list(reversed(range(timesteps)))
        tab = lambda name: [float(h[name][t]) for t in ts]
        tables = {k: tab(k) for k in ('sqrt_recip_alphas_cumprod', 'sqrt_recipm1_alphas_cumprod', 'posterior_mean_coef1',
                                      'posterior_mean_coef2')}
        tables['std'] = [0.0 if t == 0 else float(np.exp(0.5 * h['posterior_log_variance_clipped'][t])) * temperature for t in ts]
        m = None
        if mask is not None:
            m = mask.to(img.dtype).expand_as(img).contiguous()
            tables['sqrt_alphas_cumprod_t'] = tab('sqrt_alphas_cumprod')
            tables['sqrt_one_minus_alphas_cumprod_t'] = tab('sqrt_one_minus_alphas_cumprod')
        logs = [j for j, t in enumerate(ts) if log_every_t and (t % log_every_t == 0 or t == timesteps - 1)]
        if getattr(self, 'device_noise', None) is not None:
            # no planes, so no bound to respect and no cut: the armed engine makes both streams in its step kernel (std carries the
            # temperature, as on the per-step route)
            with self.engine.loop_noise(self.device_noise, self.noise_first_sample, 0, 1., repeat_noise):
                img, x_inter = self.engine.sample_ancestral(img, ctx, ts, tables, mask=m, x0=None if mask is None else x0, log_steps=logs,
                                                            control_scales=control_scales, flags=flags)
            return img, [] if x_inter is None else list(x_inter)
        inter = []
        step_bytes = img.numel() * 4 * (1 if mask is None else 2)
        for a, b in plan_noise_segments(len(ts), step_bytes, getattr(self, 'max_loop_noise_bytes', 256 << 20)):
            sn = torch.empty(b - a, *img.shape, device=img.device, dtype=torch.float32)
            qn = None if mask is None else torch.empty_like(sn)
            for k in range(b - a):
                sn[k] = _randn((1, *img.shape[1:]) if repeat_noise else img.shape, img.device)      # p_sample (expanded by the copy)
                if qn is not None:
                    qn[k] = torch.randn_like(x0)                                                    # q_sample(x0, ts)
            img, x_inter = self.engine.sample_ancestral(img, ctx, ts[a:b], {k: v[a:b] for k, v in tables.items()}, step_noise=sn,
                                                        mask=m, x0=None if mask is None else x0, q_noise=qn,
                                                        log_steps=[j - a for j in logs if a <= j < b],
                                                        control_scales=control_scales, flags=flags)
            if x_inter is not None:
                inter += list(x_inter)
            del sn, qn          # given back (in stream order) before the next segment's are taken: one bound of noise at a time, not two
        return img, inter

    def p_sample_loop(self, cond, shape, return_intermediates=False, x_T=None, verbose=True, callback=None,
                      timesteps=None, quantize_denoised=False, mask=None, x0=None, img_callback=None, start_T=None,
                      log_every_t=None, **kwargs):
        """ddpm.py:1382-1430.  A model built with device_loop=True hands the walk to the engine (fgdm_sample_ancestral) when nothing
        asked for needs the host between steps (_ancestral_plan); everything else, and the default, is the per-step loop below."""
        if quantize_denoised:
            raise NotImplementedError('quantize_denoised needs a VQ first stage')
        log_every_t = log_every_t or self.log_every_t
        b = shape[0]
        img = _randn(shape, self.device) if x_T is None else x_T.to(self.device, torch.float32)
        inter = [img]
        timesteps = self.num_timesteps if timesteps is None else timesteps
        if start_T is not None:
            timesteps = min(timesteps, start_T)
        if mask is not None:
            assert x0 is not None and x0.shape[2:3] == mask.shape[2:3]
        plan = self._ancestral_plan(cond, img, timesteps, mask, x0, bool(callback or img_callback), kwargs)
        if plan is not None:
            img, logged = self._device_ancestral(plan, img, timesteps, mask, x0, log_every_t if return_intermediates else None, **kwargs)
            return (img, inter + logged) if return_intermediates else img
        generated = getattr(self, 'device_noise', None) is not None
        for i in reversed(range(0, timesteps)):
            ts = torch.full((b,), i, device=self.device, dtype=torch.long)
            self._noise_pos = timesteps - 1 - i
            img = self.p_sample(img, cond, ts, clip_denoised=self.clip_denoised, **kwargs)
            if mask is not None:
                img_orig = self.q_sample(x0, ts, self._generated(_lib.NOISE_STREAM_Q, x0.shape)) if generated else self.q_sample(x0, ts)
                img = _k.mask_blend(img_orig.contiguous(), img.contiguous(),
                                    mask.to(img.dtype).expand_as(img).contiguous())
            if i % log_every_t == 0 or i == timesteps - 1:
                inter.append(img)
            if callback:
                callback(i)
            if img_callback:
                img_callback(img, i)
        return (img, inter) if return_intermediates else img

    def sample(self, cond, batch_size=16, return_intermediates=False, x_T=None, verbose=True, timesteps=None,
               quantize_denoised=False, mask=None, x0=None, shape=None, **kwargs):
        if shape is None:
            shape = (batch_size, self.channels, self.image_size, self.image_size)
        if cond is not None:
            if isinstance(cond, dict):
                cond = {k: (v[:batch_size] if not isinstance(v, list) else [u[:batch_size] for u in v])
                        for k, v in cond.items()}
            else:
                cond = [c[:batch_size] for c in cond] if isinstance(cond, list) else cond[:batch_size]
        return self.p_sample_loop(cond, shape, return_intermediates=return_intermediates, x_T=x_T, verbose=verbose,
                                  timesteps=timesteps, quantize_denoised=quantize_denoised, mask=mask, x0=x0, **kwargs)


class ControlLDM(LatentDiffusion):
    """controlnet/cldm/cldm.py:816-849.  Several control models (BASELINE configs 4/5) are an extension: their
    residual lists are summed; cond['c_concat'] then carries one hint per control model."""

    def __init__(self, unet_config=None, n_controlnets=1, only_mid_control=False, control_key='hint',
                 control_stage_config=None, **kw):
        kw.setdefault('use_adapter', False)       # ControlledUnetModel is the plain SD UNet (cldm.py:26)
        kw.setdefault('image_size', 64)
        self._check_control_stage(unet_config, control_stage_config)
        super().__init__(unet_config=unet_config, n_controlnets=n_controlnets, **kw)
        self.control_key = control_key
        self.only_mid_control = only_mid_control
        self.n_controlnets = n_controlnets
        self.control_scales = [1.0] * 13

    @staticmethod
    def _check_control_stage(unet_config, control_stage_config):
        """cldm_v15_canny.yaml:21-36: control_stage_config must describe the twin of the UNet's encoder"""
        if control_stage_config is None:
            return
        ckind, ccfg, cflags = _cfg.unet_params(control_stage_config)
        _, ucfg, _ = _cfg.unet_params(unet_config)
        ucfg = dict(_k.SD_V1 if ucfg is None else ucfg)
        sd2 = _cfg._SD2_KEYS       # absent from a cfg when unset: compared by their defaults, so a twin must match in them too
        diff = [k for k in list(ccfg) + [k for k in sd2 if k not in ccfg] if k != 'out_channels' and
                tuple(np.atleast_1d(ccfg.get(k, sd2.get(k)))) != tuple(np.atleast_1d(ucfg.get(k, sd2.get(k))))]
        if ckind not in (None, 'controlnet') or diff or cflags.get('hint_channels', 3) != 3:
            raise NotImplementedError(f'control_stage_config must be a ControlNet matching unet_config (differs in {diff})')

    @classmethod
    def engine_args(cls, unet_config=None, n_controlnets=1, control_stage_config=None, **kw):
        kw.setdefault('use_adapter', False)
        cls._check_control_stage(unet_config, control_stage_config)
        return super().engine_args(unet_config=unet_config, n_controlnets=n_controlnets, **kw)

    def _scales(self):
        sc = list(self.control_scales)
        if len(sc) == 13:
            sc = sc * self.n_controlnets
        assert len(sc) == 13 * self.n_controlnets, 'control_scales: 13 per control model'
        return sc

    def apply_model(self, x_noisy, t, cond, *args, **kwargs):
        assert isinstance(cond, dict)
        ctx = self._context(cond)
        hints = cond.get('c_concat')
        flags = _lib.FLAG_ONLY_MID_CONTROL if self.only_mid_control else 0
        if kwargs.get('cfg_pairs', False):           # set by the samplers for cat([x] * 2) batches sharing one hint
            flags |= _lib.FLAG_CFG_PAIRS
        if hints is None:
            return self.engine.apply_model(x_noisy, t, ctx, flags=flags | _lib.FLAG_NO_CONTROL)
        if self.n_controlnets == 1:
            hints = [hints[0] if len(hints) == 1 else torch.cat(hints, 1)]     # torch.cat(cond['c_concat'], 1)
        assert len(hints) == self.n_controlnets
        for k, h in enumerate(hints):
            self.engine.set_hint(k, h)
        return self.engine.apply_model(x_noisy, t, ctx, control_scales=self._scales(), flags=flags)

    def get_unconditional_conditioning(self, N):
        return self.get_learned_conditioning([""] * N)
