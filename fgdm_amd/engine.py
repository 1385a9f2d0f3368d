"""Python handle on the HIP engine (libfgdm_hip.so).  torch is used only as a container for device
memory and for the current HIP stream; all arithmetic happens in the hand-written kernels."""
import ctypes as C
import os
from collections import OrderedDict

import numpy as np
import torch

from . import _lib

SD_V1 = dict(in_channels=4, out_channels=4, model_channels=320, attention_resolutions=(4, 2, 1),
             num_res_blocks=2, channel_mult=(1, 2, 4, 4), num_heads=8, context_dim=768)


# AutoencoderKL ddconfig of the shipped configs (models/config.yaml:55-69)
SD_VAE = dict(ch=128, out_ch=3, ch_mult=(1, 2, 4, 4), num_res_blocks=2, attn_resolutions=(), z_channels=4)


# text tower of openai/clip-vit-large-patch14 (FrozenCLIPEmbedder's default `version`)
SD_CLIP = dict(vocab_size=49408, hidden_size=768, intermediate_size=3072, num_hidden_layers=12,
               num_attention_heads=12, max_position_embeddings=77)


def make_config(cfg=None, use_adapter=False, n_controlnets=0, hint_channels=3, workspace_bytes=0, vae=None, clip=None,
                num_prompts=1, vae_encoder=False):
    """fgdm_config from the reference's UNetModel kwargs (models/config.yaml:33-48; SD-2.x nodes carry `num_head_channels` with
    `num_heads=-1`, and `use_linear_in_transformer`); `vae`: None (no first-stage
    decoder), True (SD_VAE) or the AutoencoderKL `ddconfig` dict; `clip`: None, True (SD_CLIP) or a CLIPTextConfig-style
    dict (text encoder in the engine); `vae_encoder`: also the first-stage ENCODER of that `vae` (AutoencoderKL.encode: the
    parameter table then lists the whole AutoencoderKL.state_dict(), encoder.* and quant_conv.* included)."""
    if vae_encoder and not vae:
        raise ValueError('vae_encoder needs the first-stage config: pass vae=True or a ddconfig dict')
    if cfg is not None and ('target' in cfg or any(k not in SD_V1 for k in cfg)):
        from . import config as _cfgmod          # {target, params} node / OmegaConf / dict with extra UNetModel kwargs
        cfg = _cfgmod.unet_params(cfg)[1]
    cfg = dict(SD_V1 if cfg is None else cfg)
    c = _lib.FgdmConfig2()
    c.in_channels = cfg['in_channels']
    c.out_channels = cfg['out_channels']
    c.model_channels = cfg['model_channels']
    c.num_res_blocks = cfg['num_res_blocks']
    cm = list(cfg['channel_mult'])
    ar = list(cfg['attention_resolutions'])
    c.n_levels = len(cm)
    for i, v in enumerate(cm):
        c.channel_mult[i] = v
    c.n_attention_resolutions = len(ar)
    for i, v in enumerate(ar):
        c.attention_resolutions[i] = v
    c.num_heads = cfg['num_heads']
    # SD-2.x networks: a fixed head WIDTH (then num_heads is -1) and nn.Linear proj_in / proj_out; absent: the SD-v1 values
    c.num_head_channels = cfg.get('num_head_channels', -1)
    c.use_linear_in_transformer = int(bool(cfg.get('use_linear_in_transformer', False)))
    c.context_dim = cfg['context_dim']
    c.use_adapter = 2 if use_adapter in ('time', 2) else int(bool(use_adapter))      # 'time' -> TimeAdapter
    c.n_controlnets = int(n_controlnets)
    c.hint_channels = hint_channels
    c.workspace_bytes = int(workspace_bytes)
    c.n_extra_adapters = int(num_prompts) - 1      # AdaptUNetModel(num_prompts=...) (openaimodel.py:947,995-999)
    if vae:
        dd = dict(SD_VAE if vae is True else vae)
        if list(dd.get('attn_resolutions', ())):
            raise ValueError('first-stage decoder: attention at up levels (attn_resolutions) is not supported')
        c.vae_ch = dd['ch']
        c.vae_n_levels = len(dd['ch_mult'])
        for i, v in enumerate(dd['ch_mult']):
            c.vae_ch_mult[i] = v
        c.vae_num_res_blocks = dd['num_res_blocks']
        c.vae_z_channels = dd['z_channels']
        c.vae_out_ch = dd['out_ch']
        if vae_encoder:
            if not dd.get('double_z', True) or dd.get('in_channels', 3) != 3:
                raise ValueError('first-stage encoder: double_z = True and in_channels = 3 are required')
            c.vae_encoder = 1
    if clip:
        cc = dict(SD_CLIP if clip is True else clip)
        c.clip_layers = cc['num_hidden_layers']
        c.clip_width = cc['hidden_size']
        c.clip_heads = cc['num_attention_heads']
        c.clip_mlp = cc['intermediate_size']
        c.clip_vocab = cc['vocab_size']
        c.clip_max_len = cc['max_position_embeddings']
    return c


def param_shapes(config):
    """OrderedDict state-dict key -> shape the engine expects (no GPU needed)."""
    lib = _lib.load()
    n = lib.fgdm_param_count(C.byref(config))
    if n < 0:
        raise ValueError(f'fgdm_param_count failed ({n}): unsupported config')
    out = OrderedDict()
    name = C.create_string_buffer(256)
    shape = (C.c_int64 * 8)()
    ndim = C.c_int()
    for i in range(n):
        rc = lib.fgdm_param_info(C.byref(config), i, name, 256, shape, C.byref(ndim))
        if rc != 0:
            raise RuntimeError(f'fgdm_param_info({i}) failed: {rc}')
        out[name.value.decode()] = tuple(int(shape[k]) for k in range(ndim.value))
    return out


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


class ContextCachePolicy:
    """Which conditioning tensor's to_k / to_v projections the engine holds (fgdm_set_context: a free, ~50 hipMallocs and a sync).
    The samplers hand the SAME tensor object to every denoising step, so registering on a miss is right -- unless the caller
    ALTERNATES two contexts (guess mode: the conditional and the unconditional call of every step,
    controlnet/cldm/ddim_hacked.py:190-191; seg2image): then one of them stays registered and the other is passed along and
    projected from the workspace on every call.  see(ctx) -> 'hit' | 'register' | 'bypass'; holding the object keeps its storage
    from being recycled under the same address, torch bumps _version on in-place writes."""

    def __init__(self, window=4):
        import collections
        self.obj, self.ver = None, -1
        self.recent = collections.deque(maxlen=window)       # (id, version) of the last contexts seen
        self.registrations = 0

    def see(self, ctx):
        key = (id(ctx), ctx._version)
        if ctx is self.obj and ctx._version == self.ver:
            verdict = 'hit'
        elif key in self.recent and any(k != key for k in self.recent):
            verdict = 'bypass'            # seen a moment ago with another context in between: an alternation, not a new prompt
        else:
            verdict = 'register'
            self.obj, self.ver = ctx, ctx._version
            self.registrations += 1
        self.recent.append(key)
        return verdict


def attention_blocks(config):
    """The UNet's transformer blocks in the order of the forward pass (csrc/model.h: input blocks, middle block, output blocks),
    as (place, ds) pairs: place in 'down' / 'mid' / 'up', ds the block's downsampling factor against the latent.  Index i of this
    list is bit i of fgdm_attention_capture.block_mask."""
    ares = {config.attention_resolutions[i] for i in range(config.n_attention_resolutions)}
    out, ds = [], 1
    for level in range(config.n_levels):
        out += [('down', ds)] * (config.num_res_blocks if ds in ares else 0)
        if level != config.n_levels - 1:
            ds *= 2
    out.append(('mid', ds))
    for level in reversed(range(config.n_levels)):
        out += [('up', ds)] * (config.num_res_blocks + 1 if ds in ares else 0)
        if level:
            ds //= 2
    return out


def resolve_attention_blocks(config, blocks=None, latent=None):
    """Block indices (sorted, unique) from what a caller names: None = every block; an index; 'down' / 'mid' / 'up'; ('down', 16)
    -- a place and a side; or a side alone as a string of digits such as '16' -- the blocks whose maps are that many cells wide
    for a latent `latent` cells wide (ptp_utils users select by place and resolution).  A bare int is an INDEX; pass the side as
    a string or in a pair.  Raises ValueError for a name that selects nothing."""
    table = attention_blocks(config)
    if blocks is None:
        return list(range(len(table)))
    if isinstance(blocks, (str, int)) or (isinstance(blocks, tuple) and len(blocks) == 2 and isinstance(blocks[0], str)):
        blocks = [blocks]

    def side_of(ds):
        if latent is None:
            raise ValueError('selecting blocks by side needs the latent side (latent=...)')
        return -(-int(latent) // ds)

    picked = set()
    for b in blocks:
        if isinstance(b, int) and not isinstance(b, bool):
            if not 0 <= b < len(table):
                raise ValueError(f'block {b}: the UNet has transformer blocks 0..{len(table) - 1}')
            hit = [b]
        elif isinstance(b, str) and b.isdigit():
            hit = [i for i, (_, ds) in enumerate(table) if side_of(ds) == int(b)]
        elif isinstance(b, str):
            hit = [i for i, (place, _) in enumerate(table) if place == b]
        else:
            place, side = b
            hit = [i for i, (pl, ds) in enumerate(table) if pl == place and side_of(ds) == int(side)]
        if not hit:
            raise ValueError(f'{b!r} names no transformer block of this UNet (places: down, mid, up)')
        picked.update(hit)
    return sorted(picked)


class AttentionCapture:
    """What Engine.capture_attention yields: the head-averaged text cross-attention maps the engine accumulates while the plan is
    set.  maps() -> {block: fp32 [rows, h, w, n_tokens] on the device}, the mean over the captured evaluations in 'sum' mode, the
    last evaluation's in 'last' mode; reset() zeroes the accumulators and the evaluation count."""

    def __init__(self, engine, blocks, tokens, rows, mode, batch=0, latent_hw=(0, 0)):
        if rows not in _lib.CAPTURE_ROWS or mode not in _lib.CAPTURE_MODES:
            raise ValueError("rows is 'cond', 'uncond' or 'all'; mode is 'sum' or 'last'")
        self.engine, self.blocks, self.mode = engine, list(blocks), mode
        self.tokens = None if tokens is None else [int(k) for k in tokens]
        self.plan = _lib.FgdmAttentionCapture()
        self.plan.struct_size = C.sizeof(self.plan)
        if self.tokens is not None:
            self._tok = (C.c_int32 * len(self.tokens))(*self.tokens)
            self.plan.tokens = C.cast(self._tok, C.POINTER(C.c_int32))
            self.plan.n_tokens = len(self.tokens)
        for b in self.blocks:
            self.plan.block_mask |= 1 << b
        self.plan.rows, self.plan.mode = _lib.CAPTURE_ROWS[rows], _lib.CAPTURE_MODES[mode]
        self.plan.batch, self.plan.latent_h, self.plan.latent_w = int(batch), int(latent_hw[0]), int(latent_hw[1])

    def __enter__(self):
        e = self.engine
        e._check(e.lib.fgdm_attention_capture_set(e.h, C.byref(self.plan)), 'fgdm_attention_capture_set')
        return self

    def __exit__(self, *exc):
        e = self.engine
        e._check(e.lib.fgdm_attention_capture_set(e.h, None), 'fgdm_attention_capture_set')
        return False

    def info(self, block):
        e = self.engine
        shape, n = (C.c_int64 * 3)(), C.c_int32()
        e._check(e.lib.fgdm_attention_capture_info(e.h, block, shape, C.byref(n)), 'fgdm_attention_capture_info')
        return tuple(int(v) for v in shape), int(n.value)

    @property
    def n_evals(self):
        return self.info(self.blocks[0])[1]

    def reset(self):
        e = self.engine
        e._check(e.lib.fgdm_attention_capture_reset(e.h, _stream()), 'fgdm_attention_capture_reset')

    def raw(self, block):
        """the accumulated plane of `block` as the engine holds it, fp32 [rows, h * w, n_tokens], divided by nothing"""
        e = self.engine
        shape, _ = self.info(block)
        out = torch.empty(shape, device=e.device, dtype=torch.float32)
        e._check(e.lib.fgdm_attention_capture_read(e.h, block, _ptr(out), _stream()), 'fgdm_attention_capture_read')
        return out

    def maps(self):
        e = self.engine
        out = {}
        for b in self.blocks:
            (rows, _, ntok), n = self.info(b)
            h, w = C.c_int32(), C.c_int32()
            e._check(e.lib.fgdm_attention_capture_block_size(e.h, b, C.byref(h), C.byref(w)), 'fgdm_attention_capture_block_size')
            m = self.raw(b).view(rows, h.value, w.value, ntok)
            out[b] = m / n if self.mode == 'sum' and n > 1 else m
        return out


class LoopNoise:
    """What Engine.loop_noise yields: while it is open the engine is armed with a fgdm_noise_plan (include/fgdm.h), and a device
    loop that is handed no step_noise / q_noise makes that noise in its step kernels.  Leaving it disarms the engine."""

    def __init__(self, engine, seed, first_sample=0, first_step=0, temperature=1., repeat_noise=False):
        self.engine = engine
        self.plan = _lib.FgdmNoisePlan()
        self.plan.struct_size = C.sizeof(self.plan)
        self.plan.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.plan.first_sample, self.plan.first_step = int(first_sample), int(first_step)
        self.plan.temperature, self.plan.repeat_noise = float(temperature), int(bool(repeat_noise))

    def __enter__(self):
        e = self.engine
        e._check(e.lib.fgdm_loop_noise_set(e.h, C.byref(self.plan)), 'fgdm_loop_noise_set')
        return self

    def __exit__(self, *exc):
        e = self.engine
        e._check(e.lib.fgdm_loop_noise_set(e.h, None), 'fgdm_loop_noise_set')
        return False


def randn(seed, stream, step, shape, first_sample=0, repeat=False, temperature=1., device=None, out=None):
    """fp32 `shape` = [B, ...] of the normals an armed device loop makes at walk position `step` on `stream` (0: the sampler's
    step noise, 1: q_sample's) for the global rows first_sample .. first_sample + B - 1 (fgdm_randn, include/fgdm.h): what the
    per-step route draws with device_noise, so both routes give the same bits.  repeat: every row is sample 0; the values are
    multiplied by temperature (one rounding)."""
    lib = _lib.load()
    if out is None:
        out = torch.empty(tuple(shape), device=device if device is not None else 'cuda', dtype=torch.float32)
    B = out.shape[0]
    rc = lib.fgdm_randn(int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream), int(step), int(first_sample), int(bool(repeat)), float(temperature),
                        _ptr(out), B, out[0].numel(), _stream())
    if rc != 0:
        raise RuntimeError(f'fgdm_randn failed: {rc}')
    return out


class Engine:
    """One engine per device: owns packed weights + activation workspace in HBM."""

    def __init__(self, cfg=None, use_adapter=False, n_controlnets=0, device=0, workspace_bytes=0, vae=None, clip=None,
                 num_prompts=1, vae_encoder=False):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError('fgdm_amd.Engine needs a GPU (MI355X); there is no CPU fallback')
        self.config = make_config(cfg, use_adapter, n_controlnets, workspace_bytes=workspace_bytes, vae=vae, clip=clip,
                                  num_prompts=num_prompts, vae_encoder=vae_encoder)
        self.has_vae = bool(vae)
        self.has_vae_encoder = bool(vae_encoder)
        self.has_clip = bool(clip)
        self.device = torch.device('cuda', device)
        torch.cuda.set_device(self.device)
        h = C.c_void_p()
        rc = self.lib.fgdm_create(C.byref(self.config), device, C.byref(h))
        if rc != 0:
            why = self.lib.fgdm_last_error(None)
            raise RuntimeError(f'fgdm_create failed ({rc}): {why.decode() if why else ""}')
        self.h = h
        self.n_controlnets = n_controlnets
        self.use_adapter = bool(use_adapter)
        self._hint_keys = [None] * n_controlnets
        self._ctx_policy = ContextCachePolicy()      # context tensor whose K/V projections the engine holds
        self._ctx_tokens = self.lib.fgdm_get_context_tokens(self.h)      # tokens per context (77 unless changed)
        self._conds_key, self._conds_keep = None, None
        self._concat_key = None
        self.concat_uploads = 0       # fgdm_set_concat calls that really stored a tensor (a repeated tensor is a cache hit)
        self.pair_calls = 0           # apply_model calls that carried FLAG_CFG_PAIRS
        self.cache_context = os.environ.get('FGDM_CONTEXT_CACHE', '1') != '0'

    def close(self):
        if getattr(self, 'h', None):
            self.lib.fgdm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            msg = self.lib.fgdm_last_error(self.h)
            raise RuntimeError(f'{what} failed ({rc}): {msg.decode() if msg else ""}')

    def capture_attention(self, blocks=None, tokens=None, rows='cond', mode='sum', latent=None, batch=0, latent_hw=(0, 0)):
        """Context manager: while it is open, every evaluation of the UNet -- per-step samplers and device loops alike --
        also accumulates the head-averaged text cross-attention maps of `blocks` (resolve_attention_blocks: indices, 'down' /
        'mid' / 'up', ('up', 16), '16' with latent=) for the context positions `tokens` (None: all).  rows: 'cond' / 'uncond' =
        that half of a CFG batch cat([uncond, cond]), 'all' = every row.  Yields an AttentionCapture.  eps is unchanged bit for
        bit; the ControlNets' cross-attentions and all self-attentions are not captured.  batch / latent_hw: give the
        evaluations' batch (2 B under CFG) and latent size to allocate now rather than at the first evaluation."""
        return AttentionCapture(self, resolve_attention_blocks(self.config, blocks, latent), tokens, rows, mode, batch, latent_hw)

    def loop_noise(self, seed, first_sample=0, first_step=0, temperature=1., repeat_noise=False):
        """Context manager: while it is open, a device loop (sample_ddim_ex, sample_plms, sample_ancestral) called without
        step_noise / q_noise makes that noise in its step kernels from a counter-based generator (fgdm_loop_noise_set): no
        [S, B,4,H,W] planes, whatever the number of steps.  first_sample: the global index of row 0 (a rank's shard offset);
        first_step: the walk position of the call's step 0; temperature / repeat_noise: of the step noise.  Tensors that are
        passed are still read.  Engine.randn gives the same numbers as a tensor."""
        return LoopNoise(self, seed, first_sample, first_step, temperature, repeat_noise)

    def randn(self, seed, stream, step, shape, first_sample=0, repeat=False, temperature=1.):
        """randn (this module) on the engine's device"""
        return randn(seed, stream, step, shape, first_sample, repeat, temperature, device=self.device)

    # ------------------------------------------------------------------ weights
    def param_shapes(self):
        return param_shapes(self.config)

    def load_tensor(self, key, value):
        if isinstance(value, torch.Tensor):
            v = value.detach()
            if v.dtype not in (torch.float32, torch.float16):
                v = v.float()
            v = v.contiguous()
            dtype = 0 if v.dtype == torch.float32 else 1
            shape = tuple(v.shape)
            ptr = C.c_void_p(v.data_ptr())
            keep = v
        else:
            a = np.ascontiguousarray(value)
            if a.dtype not in (np.float32, np.float16):
                a = a.astype(np.float32)
            dtype = 0 if a.dtype == np.float32 else 1
            shape = a.shape
            ptr = a.ctypes.data_as(C.c_void_p)
            keep = a
        sh = (C.c_int64 * len(shape))(*shape)
        rc = self.lib.fgdm_load_tensor(self.h, key.encode(), ptr, dtype, sh, len(shape))
        del keep
        self._check(rc, f'fgdm_load_tensor({key})')

    def load_state_dict(self, sd, strict=True):
        """Same keys as the reference checkpoints (model.diffusion_model.*, control_model.*); extra keys
        (first_stage_model.*, cond_stage_model.* ...) are ignored like load_state_dict(strict=False)."""
        want = self.param_shapes()
        missing = [k for k in want if k not in sd]
        if strict and missing:
            raise KeyError(f'{len(missing)} parameters missing, e.g. {missing[:3]}')
        for k in want:
            if k in sd:
                self.load_tensor(k, sd[k])
        return missing

    def finalize(self):
        self._check(self.lib.fgdm_finalize_weights(self.h), 'fgdm_finalize_weights')
        self._ctx_policy = ContextCachePolicy()
        self._hint_keys = [None] * self.n_controlnets
        self._conds_key, self._conds_keep = None, None

    # ------------------------------------------------------------------ weight updates of a finalized engine (include/fgdm.h)
    def _forget_derived(self):
        """the engine dropped what it had computed from weights (registered context, hint features, adapter conds): the next
        call hands each over again instead of taking a cache hit"""
        self._ctx_policy = ContextCachePolicy()
        self._hint_keys = [None] * self.n_controlnets
        self._conds_key, self._conds_keep = None, None

    def weights_snapshot(self, keys):
        keys = [k.encode() for k in keys]
        arr = (C.c_char_p * len(keys))(*keys)
        self._check(self.lib.fgdm_weights_snapshot(self.h, arr, len(keys)), 'fgdm_weights_snapshot')

    def weights_snapshot_bytes(self):
        return int(self.lib.fgdm_weights_snapshot_bytes(self.h))

    def weights_restore(self):
        self._check(self.lib.fgdm_weights_restore(self.h, _stream()), 'fgdm_weights_restore')
        self._forget_derived()

    def weights_begin_update(self):
        self._check(self.lib.fgdm_weights_begin_update(self.h), 'fgdm_weights_begin_update')

    def weights_update_tensor(self, key, value):
        """one parameter of the update: an fp32 tensor on the engine's device (the producing stream is synchronised here)"""
        v = value.detach().to(self.device, torch.float32).contiguous()
        torch.cuda.current_stream().synchronize()
        sh = (C.c_int64 * v.dim())(*v.shape)
        self._check(self.lib.fgdm_weights_update_tensor(self.h, key.encode(), _ptr(v), sh, v.dim()), f'fgdm_weights_update_tensor({key})')

    def weights_commit_update(self):
        try:
            self._check(self.lib.fgdm_weights_commit_update(self.h, _stream()), 'fgdm_weights_commit_update')
        finally:
            self._forget_derived()

    # ------------------------------------------------------------------ forward
    def set_hint(self, cn, hint):
        """hint fp32 NCHW [B,3,8H,8W] in [0,1]; cached until a different tensor is given.  The source object is kept
        alive with the key, so its address and version counter cannot be recycled by another tensor."""
        key = (id(hint), hint.data_ptr(), hint._version, tuple(hint.shape))
        if self._hint_keys[cn] is not None and self._hint_keys[cn][0] == key:
            return
        dev = hint.to(self.device, torch.float32).contiguous()
        B, _, Hh, Wh = dev.shape
        self._check(self.lib.fgdm_set_hint(self.h, cn, _ptr(dev), B, Hh, Wh, _stream()), 'fgdm_set_hint')
        self._hint_keys[cn] = (key, hint)

    def set_adapter_conds(self, conds):
        """AdaptUNetModel's `conds`: list of fp32 NCHW [B,4,H,W] latents (or None); their summed adapter features are
        computed once and reused until a different list is given."""
        if not conds:
            if self._conds_key is not None:
                self._check(self.lib.fgdm_set_adapter_conds(self.h, None, 0, 0, 0, 0, _stream()), 'fgdm_set_adapter_conds')
                self._conds_key, self._conds_keep = None, None
            return
        key = tuple((id(c), c._version, tuple(c.shape)) for c in conds)
        if key == self._conds_key:
            return
        dev = [c.to(self.device, torch.float32).contiguous() for c in conds]
        B, _, H, W = dev[0].shape
        ptrs = (C.c_void_p * len(dev))(*[c.data_ptr() for c in dev])
        self._check(self.lib.fgdm_set_adapter_conds(self.h, ptrs, len(dev), B, H, W, _stream()), 'fgdm_set_adapter_conds')
        self._conds_key, self._conds_keep = key, list(conds)

    def set_concat(self, c_concat):
        """c_concat of an engine whose UNet reads cat([x, c_concat], 1) (in_channels > 4; DiffusionWrapper 'hybrid', ddpm.py:1838-
        1841): fp32 NCHW [B, in_channels - 4, H, W], stored once as fp16 NHWC and kept until a different tensor (object, version
        or shape) is given; None drops it.  B is the batch of the later apply_model calls, or half of it (the two halves of a
        classifier-free-guidance batch then share the rows).  The source object is kept alive with the key, as for set_hint."""
        if c_concat is None:
            self._check(self.lib.fgdm_set_concat(self.h, None, 0, 0, 0, 0, _stream()), 'fgdm_set_concat')
            self._concat_key = None
            return
        key = (id(c_concat), c_concat.data_ptr(), c_concat._version, tuple(c_concat.shape))
        if self._concat_key is not None and self._concat_key[0] == key:
            return
        self._concat_key = None       # a refused call leaves nothing that a later hit could vouch for
        dev = c_concat.to(self.device, torch.float32).contiguous()
        B, Cc, H, W = dev.shape
        self._check(self.lib.fgdm_set_concat(self.h, _ptr(dev), B, Cc, H, W, _stream()), 'fgdm_set_concat')
        self._concat_key = (key, c_concat)
        self.concat_uploads += 1

    def set_context_tokens(self, tokens):
        """Token count of every context handed over from now on (cat(c_crossattn, 1) may hold several 77-token parts,
        ddpm.py:1835-1837 / hack.py:23-68).  A changed count drops the engine's registered projections, so the cache policy
        starts afresh as well: the next tensor is a new context even if it is an object seen before."""
        tokens = int(tokens)
        if tokens != self._ctx_tokens:
            self._check(self.lib.fgdm_set_context_tokens(self.h, tokens), 'fgdm_set_context_tokens')
            self._ctx_tokens = tokens
            self._ctx_policy = ContextCachePolicy()

    def apply_model(self, x, t, ctx, control_scales=None, flags=0, pcond=None, out=None):
        x = x.to(self.device, torch.float32).contiguous()
        t_int = t_flt = None
        if t.is_floating_point():        # fractional timesteps (DPM-Solver)
            t_flt = t.to(self.device, torch.float32).contiguous()
        else:
            t_int = t.to(self.device, torch.int64).contiguous()
        B, Cc, H, W = x.shape
        if Cc != 4 or ctx.shape[0] != B or t.shape[0] != B:
            raise ValueError(f'apply_model: x {tuple(x.shape)}, t {tuple(t.shape)}, context {tuple(ctx.shape)} do not agree')
        self.set_context_tokens(ctx.shape[1])
        # The conditioning is the same tensor OBJECT in every denoising step: its to_k / to_v projections are computed
        # once (fgdm_set_context) and reused while that object is unmodified (torch bumps _version on in-place writes;
        # holding the object keeps its storage from being recycled under the same address).
        ctx_arg = None
        if self.cache_context and ctx.is_cuda and ctx.dtype == torch.float32 and ctx.is_contiguous():
            verdict = self._ctx_policy.see(ctx)
            if verdict == 'register':
                self._check(self.lib.fgdm_set_context(self.h, _ptr(ctx), B, _stream()), 'fgdm_set_context')
            elif verdict == 'bypass':
                ctx_arg = ctx
        else:
            ctx_arg = ctx.to(self.device, torch.float32).contiguous()
        eps = torch.empty_like(x) if out is None else out
        sc = None
        if control_scales is not None:
            sc = torch.as_tensor(control_scales, dtype=torch.float32).flatten()
            assert sc.numel() == 13 * self.n_controlnets
            sc_host = sc.numpy().copy()
            sc_ptr = sc_host.ctypes.data_as(C.c_void_p)
        else:
            sc_ptr = C.c_void_p(0)
        if pcond is not None:
            if tuple(pcond.shape) != tuple(x.shape):
                raise ValueError(f'pcond / control shape {tuple(pcond.shape)} must equal the latent batch {tuple(x.shape)}')
            pcond = pcond.to(self.device, torch.float32).contiguous()
        rc = self.lib.fgdm_apply_model(self.h, _ptr(x), _ptr(t_int), _ptr(t_flt), _ptr(ctx_arg), _ptr(pcond), sc_ptr, B, H, W,
                                       flags, _ptr(eps), _stream())
        self._check(rc, 'fgdm_apply_model')
        self.pair_calls += bool(flags & _lib.FLAG_CFG_PAIRS)
        return eps

    def clip_encode(self, ids, clip_skip=0):
        """CLIPTextModel(input_ids=ids).last_hidden_state: int64 ids [B, T<=77] -> fp32 [B, T, 768] on the device.
        clip_skip > 1: final_layer_norm(hidden_states[-clip_skip]) instead (controlnet/cldm/hack.py:40-45)."""
        ids = torch.as_tensor(ids).to(self.device, torch.int64).contiguous()
        B, T = ids.shape
        out = torch.empty(B, T, self.config.clip_width, device=self.device, dtype=torch.float32)
        self._check(self.lib.fgdm_clip_encode_skip(self.h, _ptr(ids), B, T, int(clip_skip), _ptr(out), _stream()),
                    'fgdm_clip_encode_skip')
        return out

    def vae_decode(self, z, scale=1.0):
        """AutoencoderKL.decode(scale * z): fp32 NCHW latents [B,4,H,W] -> fp32 NCHW images [B,3,8H,8W]."""
        z = z.to(self.device, torch.float32).contiguous()
        B, Cc, H, W = z.shape
        assert Cc == 4
        f = 1 << (self.config.vae_n_levels - 1)
        img = torch.empty(B, self.config.vae_out_ch, H * f, W * f, device=self.device, dtype=torch.float32)
        rc = self.lib.fgdm_vae_decode(self.h, _ptr(z), B, H, W, float(scale), _ptr(img), _stream())
        self._check(rc, 'fgdm_vae_decode')
        return img

    def vae_decode_patches(self, z, scale, ks, stride, f, w_pix, w_tie, max_crops_per_pass=0):
        """decode_first_stage with split_input_params (ddpm.py:841-878): z [B,4,H,W] in (kh, kw) latent crops every `stride`,
        each decoded like vae_decode and blended with w_pix [f kh, f kw], w_tie [L] (device fp32, fgdm_amd/patches.py) into
        fp32 [B,3,f H,f W].  max_crops_per_pass bounds the crops decoded together (0: the decoder's own rule)."""
        z = z.to(self.device, torch.float32).contiguous()
        B, Cc, H, W = z.shape
        assert Cc == 4
        w_pix, w_tie = _weights(w_pix, w_tie, self.device, (H, W, ks, stride, int(f)))
        img = torch.empty(B, self.config.vae_out_ch, H * f, W * f, device=self.device, dtype=torch.float32)
        rc = self.lib.fgdm_vae_decode_patches(self.h, _ptr(z), B, H, W, float(scale), ks[0], ks[1], stride[0], stride[1], int(f),
                                              _ptr(w_pix), _ptr(w_tie), int(max_crops_per_pass), _ptr(img), _stream())
        self._check(rc, 'fgdm_vae_decode_patches')
        return img

    def apply_model_patches(self, x, t, ctx, ks, stride, w_pix, w_tie, max_crops_per_pass=0, flags=0):
        """apply_model with split_input_params (ddpm.py:1046-1128, text branch): the UNet on every (kh, kw) crop of x with the
        same t and context, blended with w_pix [kh, kw], w_tie [L].  The context is handed over explicitly on every call (the
        engine's registered context, and this handle's cache policy, are left alone)."""
        x = x.to(self.device, torch.float32).contiguous()
        t_int = t_flt = None
        if t.is_floating_point():
            t_flt = t.to(self.device, torch.float32).contiguous()
        else:
            t_int = t.to(self.device, torch.int64).contiguous()
        B, Cc, H, W = x.shape
        if Cc != 4 or ctx.shape[0] != B or t.shape[0] != B:
            raise ValueError(f'apply_model_patches: x {tuple(x.shape)}, t {tuple(t.shape)}, context {tuple(ctx.shape)} do not agree')
        self.set_context_tokens(ctx.shape[1])
        ctx = ctx.to(self.device, torch.float32).contiguous()
        w_pix, w_tie = _weights(w_pix, w_tie, self.device, (H, W, ks, stride, 1))
        eps = torch.empty_like(x)
        rc = self.lib.fgdm_apply_model_patches(self.h, _ptr(x), _ptr(t_int), _ptr(t_flt), _ptr(ctx), B, H, W, ks[0], ks[1],
                                               stride[0], stride[1], _ptr(w_pix), _ptr(w_tie), int(max_crops_per_pass),
                                               int(flags), _ptr(eps), _stream())
        self._check(rc, 'fgdm_apply_model_patches')
        return eps

    def unfold(self, x, ks, stride, l0=0, n=None, out=None):
        return unfold(x.to(self.device), ks, stride, l0, n, out)

    def fold_weighted(self, crops, w_pix, w_tie, size, stride, crops_per_pass=0, out=None):
        return fold_weighted(crops.to(self.device), w_pix, w_tie, size, stride, crops_per_pass, out)

    def vae_encode(self, image):
        """AutoencoderKL.encode(image).parameters: fp32 NCHW images [B,3,H,W] in [-1,1] -> fp32 NCHW moments [B,8,H/8,W/8]
        (channels 0-3 the posterior mean, 4-7 its log-variance).  Needs an engine built with vae_encoder=True."""
        image = image.to(self.device, torch.float32).contiguous()
        B, Cc, H, W = image.shape
        if Cc != 3:
            raise ValueError(f'vae_encode: image {tuple(image.shape)} must have 3 channels')
        f = 1 << (self.config.vae_n_levels - 1)
        moments = torch.empty(B, 2 * self.config.vae_z_channels, H // f, W // f, device=self.device, dtype=torch.float32)
        rc = self.lib.fgdm_vae_encode(self.h, _ptr(image), B, H, W, _ptr(moments), _stream())
        self._check(rc, 'fgdm_vae_encode')
        return moments

    def posterior_sample(self, moments, noise=None, scale=1.0):
        """scale * DiagonalGaussianDistribution(moments).sample() with the given noise, or scale * mode() without."""
        return posterior_sample(moments.to(self.device), None if noise is None else noise.to(self.device), scale)

    def run_block(self, prefix, x, emb=None, ctx=None, x_skip=None):
        """One block (or one layer of a block, or the FG-DM adapter) of the loaded graph by state-dict prefix, e.g.
        'model.diffusion_model.input_blocks.4.' / '...input_blocks.4.1.' / 'model.diffusion_model.adapter.'.
        fp32 NCHW in and out; returns a flat fp32 tensor (the caller knows the block's output shape)."""
        f32 = lambda v: None if v is None else v.to(self.device, torch.float32).contiguous()
        x, emb, ctx, x_skip = f32(x), f32(emb), f32(ctx), f32(x_skip)
        if ctx is not None:
            self.set_context_tokens(ctx.shape[1])
        B, Cc, H, W = x.shape
        cap = 4 * B * 1280 * 4 * H * W            # generous: an Upsample quadruples the pixels
        out = torch.empty(cap, device=self.device, dtype=torch.float32)
        n = C.c_int64(0)
        rc = self.lib.fgdm_run_block(self.h, prefix.encode(), _ptr(x), Cc, _ptr(x_skip), 0 if x_skip is None else x_skip.shape[1],
                                     _ptr(emb), _ptr(ctx), B, H, W, _ptr(out), cap, C.byref(n), _stream())
        self._check(rc, f'fgdm_run_block({prefix})')
        return out[:n.value]

    def controlnet(self, cn, x, t, ctx):
        """The 13 ControlNet residuals (fp32 NCHW), for inspection / tests."""
        x = x.to(self.device, torch.float32).contiguous()
        t = t.to(self.device, torch.int64).contiguous()
        ctx = ctx.to(self.device, torch.float32).contiguous()
        self.set_context_tokens(ctx.shape[1])
        B, _, H, W = x.shape
        shapes = self.control_shapes(B, H, W)
        total = sum(int(np.prod(s)) for s in shapes)
        buf = torch.empty(total, device=self.device, dtype=torch.float32)
        rc = self.lib.fgdm_controlnet(self.h, cn, _ptr(x), _ptr(t), _ptr(ctx), B, H, W, _ptr(buf), total, _stream())
        self._check(rc, 'fgdm_controlnet')
        outs, off = [], 0
        for s in shapes:
            n = int(np.prod(s))
            outs.append(buf[off:off + n].view(*s))
            off += n
        return outs

    # ------------------------------------------------------------------ built-in kernel timer
    PROFILE_CLASSES = ('igemm', 'attention', 'norm', 'im2col')

    def profile_begin(self, stride=1):
        """Bracket every `stride`-th kernel launch with HIP events (1 = every launch)."""
        self._check(self.lib.fgdm_profile_begin(self.h, int(stride)), 'fgdm_profile_begin')

    def profile_end(self):
        """{class: dict(ms, launches, work)}; work = algorithmic flops (igemm, attention) or bytes (norm, im2col)."""
        buf = (C.c_double * 16)()
        self._check(self.lib.fgdm_profile_end(self.h, buf), 'fgdm_profile_end')
        return {n: dict(ms=buf[4 * i], launches=int(buf[4 * i + 1]), work=buf[4 * i + 2], bytes=buf[4 * i + 3])
                for i, n in enumerate(self.PROFILE_CLASSES)}

    def workspace_stats(self):
        a, b = C.c_int64(), C.c_int64()
        self._check(self.lib.fgdm_workspace_stats(self.h, C.byref(a), C.byref(b)), 'fgdm_workspace_stats')
        return dict(peak_bytes=a.value, reserved_bytes=b.value)

    def launch_stats(self):
        """Grouped twin launches since the engine was created: replayed launches, fused launches, problems in fused launches."""
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        self._check(self.lib.fgdm_launch_stats(self.h, C.byref(a), C.byref(b), C.byref(c)), 'fgdm_launch_stats')
        return dict(replayed_launches=a.value, fused_launches=b.value, fused_problems=c.value)

    def control_shapes(self, B, H, W):
        c = self.config
        mc = c.model_channels
        shapes = [(B, mc, H, W)]
        ch, h, w = mc, H, W
        for level in range(c.n_levels):
            for _ in range(c.num_res_blocks):
                ch = mc * c.channel_mult[level]
                shapes.append((B, ch, h, w))
            if level != c.n_levels - 1:
                h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
                shapes.append((B, ch, h, w))
        shapes.append((B, ch, h, w))
        return shapes

    def sample_ddim(self, x_T, cond, uncond, cfg_scale, timesteps, alphas, alphas_prev, sqrt_one_minus_alphas,
                    control_scales=None, flags=0):
        """Whole eta=0 DDIM loop on the device; returns the final latent (x_T is not modified)."""
        def legacy(p):      # the positional entry of the first ABI version: kept exercised
            f32, i64 = C.POINTER(C.c_float), C.POINTER(C.c_int64)
            return self.lib.fgdm_sample_ddim(self.h, p.x, p.cond, p.uncond, p.cfg_scale, p.S, C.cast(p.timesteps, i64), C.cast(p.alphas, f32),
                                             C.cast(p.alphas_prev, f32), C.cast(p.sqrt_one_minus_alphas, f32), p.control_scales, p.B, p.H,
                                             p.W, p.flags, _stream())
        S = len(timesteps)
        return self._device_loop('sample_ddim', _lib.FgdmDdimParams(), x_T, cond, uncond, None, 'S', S,
                                 dict(timesteps=(timesteps, C.c_int64, S), alphas=alphas, alphas_prev=alphas_prev,
                                      sqrt_one_minus_alphas=sqrt_one_minus_alphas), control_scales=control_scales, call=legacy,
                                 cfg_scale=float(cfg_scale), flags=int(flags))[0]

    def sample_ddim_ex(self, x_T, cond, uncond, cfg_scale, timesteps, alphas, alphas_prev, sqrt_one_minus_alphas, sigmas=None,
                       cfg_scales=None, step_noise=None, mask=None, x0=None, q_noise=None, sqrt_alphas_cumprod_t=None,
                       sqrt_one_minus_alphas_cumprod_t=None, log_steps=(), control_scales=None, flags=0, out=None,
                       x_inter_out=None, pred_x0_out=None):
        """The whole DDIM loop on the device with every option of fgdm_sample_ddim_ex (include/fgdm.h): the S-entry schedule
        tables (timesteps ... sigmas, and q_sample's two coefficient tables with a mask) in ddim_timesteps order like
        sample_ddim's; cfg_scales [S], step_noise / q_noise [S, B,4,H,W] and log_steps in WALK order (slot i: the i-th step that
        runs).  Returns (x, x_inter, pred_x0): the final latent and the two [len(log_steps), B,4,H,W] intermediates (None without
        log steps).  x_T is not modified; out / x_inter_out / pred_x0_out: caller-owned device buffers to use instead of new ones."""
        S = len(timesteps)
        return self._device_loop('sample_ddim_ex', _lib.FgdmDdimParams(), x_T, cond, uncond, out, 'S', S,
                                 dict(timesteps=(timesteps, C.c_int64, S), alphas=alphas, alphas_prev=alphas_prev,
                                      sqrt_one_minus_alphas=sqrt_one_minus_alphas, sigmas=sigmas, cfg_scales=cfg_scales,
                                      sqrt_alphas_cumprod_t=sqrt_alphas_cumprod_t, sqrt_one_minus_alphas_cumprod_t=sqrt_one_minus_alphas_cumprod_t),
                                 dict(step_noise=(step_noise, (S,)), q_noise=(q_noise, (S,)), mask=(mask, ()), x0=(x0, ())),
                                 (log_steps, dict(x_inter_out=x_inter_out, pred_x0_out=pred_x0_out)), control_scales,
                                 cfg_scale=float(cfg_scale), flags=int(flags))

    def _loop_args(self, name, x_T, cond, uncond, out):
        """the state and the conditionings of a device loop on the engine's device, as sample_ddim_ex prepares them"""
        dev = lambda v: None if v is None else v.to(self.device, torch.float32).contiguous()
        x = x_T.to(self.device, torch.float32).clone().contiguous() if out is None else out.copy_(x_T)
        cond, uncond = dev(cond), dev(uncond)
        if uncond is not None and tuple(uncond.shape) != tuple(cond.shape):      # one cat([uncond, cond]) batch (ddim.py:222-226)
            raise ValueError(f'{name}: cond {tuple(cond.shape)} and uncond {tuple(uncond.shape)} must agree')
        self.set_context_tokens(cond.shape[1])
        return x, cond, uncond

    @staticmethod
    def _table(name, keep, a, count, ctype=C.c_float, conv=float):
        """a host table of `count` entries for a parameter struct; `keep` holds the array while the call runs"""
        if a is None:
            return None
        if len(a) != count:
            raise ValueError(f'{name}: a table of {len(a)} entries where {count} are needed')
        keep.append((ctype * count)(*[conv(v) for v in a]))
        return C.cast(keep[-1], C.c_void_p)

    def _run_loop(self, name, p, keep, control_scales, call=None):
        """control_scales into the parameter struct `p`, then the native loop fgdm_<name> (or `call(p)`: the legacy entry); `keep`
        holds host arrays while it runs"""
        p.struct_size = C.sizeof(p)
        if control_scales is not None:
            keep.append(np.asarray(control_scales, dtype=np.float32).ravel().copy())
            p.control_scales = keep[-1].ctypes.data_as(C.c_void_p)
        rc = call(p) if call else getattr(self.lib, 'fgdm_' + name)(self.h, C.byref(p), _stream())
        self._ctx_policy = ContextCachePolicy()      # the device-side loop registered its own context
        self._check(rc, 'fgdm_' + name)

    def _log_args(self, name, p, keep, x, log_steps, outs):
        """log_steps / n_log / the log planes of a loop's struct.  outs: field -> caller-owned buffer or None.  Returns the
        [len(log_steps), B,4,H,W] plane of every field (None without log steps)."""
        p.n_log = len(log_steps)
        if not p.n_log:
            return [None] * len(outs)
        planes = [torch.empty(p.n_log, *x.shape, device=self.device, dtype=torch.float32) if v is None else v for v in outs.values()]
        p.log_steps = self._table(name, keep, log_steps, p.n_log, C.c_int32, int)
        for k, v in zip(outs, planes):
            setattr(p, k, _ptr(v))
        return planes

    def _device_loop(self, name, p, x_T, cond, uncond, out, count_field, count, tables, tensors=None, logs=None, control_scales=None,
                     call=None, **scalars):
        """What every device loop does around its native entry fgdm_<name>: the state and the conditionings (_loop_args), then into
        the parameter struct `p` the device tensors (field -> (tensor or None, leading dims in front of x's shape)), the host tables
        in the caller's order (field -> `count` floats or None, or (values, ctype, entries) for another type or length; values may
        be a function that is called at its turn), the log group (log_steps, {field: caller-owned plane or None}) of the loops that
        have one, the sizes and the scalar fields; then the call.  Returns (x, *log planes)."""
        x, cond, uncond = self._loop_args(name, x_T, cond, uncond, out)
        keep = []      # what the struct points into: converted tensors and host arrays, held until the call has returned
        for k, (v, lead) in (tensors or {}).items():
            v = None if v is None else v.to(self.device, torch.float32).contiguous()
            if v is not None and tuple(v.shape) != (*lead, *x.shape):
                raise ValueError(f'{name}: {k} {tuple(v.shape)} must be {(*lead, *x.shape)}')
            keep.append(v)
            setattr(p, k, _ptr(v))
        for k, spec in tables.items():
            a, ctype, n = spec if isinstance(spec, tuple) else (spec, C.c_float, count)
            setattr(p, k, self._table(name, keep, a() if callable(a) else a, n, ctype, float if ctype is C.c_float else int))
        planes = self._log_args(name, p, keep, x, *logs) if logs else []
        p.x, p.cond = _ptr(x), _ptr(cond)
        if uncond is not None:
            p.uncond = _ptr(uncond)
        _, _, H, W = x.shape
        for k, v in dict(scalars, B=x.shape[0], H=H, W=W, **{count_field: count}).items():
            setattr(p, k, v)
        self._run_loop(name, p, keep, control_scales, call)
        return (x, *planes)

    def sample_plms(self, x_T, cond, uncond, cfg_scale, timesteps, alphas, alphas_prev, sqrt_one_minus_alphas, mask=None, x0=None,
                    q_noise=None, sqrt_alphas_cumprod_t=None, sqrt_one_minus_alphas_cumprod_t=None, log_steps=(),
                    control_scales=None, flags=0, out=None, x_inter_out=None, pred_x0_out=None):
        """The whole PLMS loop on the device (fgdm_sample_plms, include/fgdm.h): the S-entry tables in ddim_timesteps order,
        q_noise [S, B,4,H,W] and log_steps in WALK order, as for sample_ddim_ex.  Returns (x, x_inter, pred_x0)."""
        S = len(timesteps)
        return self._device_loop('sample_plms', _lib.FgdmPlmsParams(), x_T, cond, uncond, out, 'S', S,
                                 dict(timesteps=(timesteps, C.c_int64, S), alphas=alphas, alphas_prev=alphas_prev,
                                      sqrt_one_minus_alphas=sqrt_one_minus_alphas, sqrt_alphas_cumprod_t=sqrt_alphas_cumprod_t,
                                      sqrt_one_minus_alphas_cumprod_t=sqrt_one_minus_alphas_cumprod_t),
                                 dict(q_noise=(q_noise, (S,)), mask=(mask, ()), x0=(x0, ())),
                                 (log_steps, dict(x_inter_out=x_inter_out, pred_x0_out=pred_x0_out)), control_scales,
                                 cfg_scale=float(cfg_scale), flags=int(flags))

    def sample_dpmpp(self, x_T, cond, uncond, cfg_scale, tables, control_scales=None, flags=0, out=None):
        """The whole DPM-Solver++ loop on the device (fgdm_sample_dpmpp, include/fgdm.h).  tables: a dict of equally long
        per-evaluation lists t_float, inv_alpha, neg_sigma_over_alpha, update_kind, c1, cm0, cm1 (fgdm_amd.samplers.dpmpp_tables).
        Returns the final latent; x_T is not modified."""
        K = len(tables['t_float'])
        return self._device_loop('sample_dpmpp', _lib.FgdmDpmppParams(), x_T, cond, uncond, out, 'n_eval', K,
                                 dict({k: tables[k] for k in ('t_float', 'inv_alpha', 'neg_sigma_over_alpha', 'c1', 'cm0', 'cm1')},
                                      update_kind=(tables['update_kind'], C.c_int32, K)), control_scales=control_scales,
                                 cfg_scale=float(cfg_scale), flags=int(flags))[0]

    def sample_dpm_solver(self, x_T, cond, uncond, cfg_scale, program, control_scales=None, flags=0, out=None):
        """A whole DPM-Solver sampling on the device (fgdm_sample_dpm_solver, include/fgdm.h).  program: the dict of equally long
        per-evaluation lists of fgdm_amd.dpm_solver.dpm_solver_program (t_float, conv_x, conv_e, slot, nterms, dest, and plane /
        coef with five entries per record).  Returns the final latent; x_T is not modified."""
        K = len(program['t_float'])

        def rows(k, check):      # program[k] as one table; at its turn, so that the row check comes behind the one-entry tables
            def flat():
                for j in check:
                    if len(program[j]) != K or any(len(r) != 5 for r in program[j]):
                        raise ValueError(f'sample_dpm_solver: {j} must hold five entries for each of the {K} records')
                return [v for r in program[k] for v in r]
            return flat
        return self._device_loop('sample_dpm_solver', _lib.FgdmDpmSolverParams(), x_T, cond, uncond, out, 'n_eval', K,
                                 dict({k: program[k] for k in ('t_float', 'conv_x', 'conv_e')},
                                      **{k: (program[k], C.c_int32, K) for k in ('slot', 'nterms', 'dest')},
                                      plane=(rows('plane', ('plane', 'coef')), C.c_int32, 5 * K), coef=(rows('coef', ()), C.c_float, 5 * K)),
                                 control_scales=control_scales, cfg_scale=float(cfg_scale), flags=int(flags))[0]

    def sample_ancestral(self, x_T, cond, timesteps, tables, step_noise=None, mask=None, x0=None, q_noise=None, log_steps=(),
                         control_scales=None, flags=0, out=None, x_inter_out=None):
        """The ancestral loop on the device (fgdm_sample_ancestral, include/fgdm.h), S = len(timesteps) steps in WALK order
        (descending t).  tables: a dict of S-entry lists sqrt_recip_alphas_cumprod, sqrt_recipm1_alphas_cumprod,
        posterior_mean_coef1, posterior_mean_coef2, std (temperature folded in, 0 where t == 0) and, with a mask,
        sqrt_alphas_cumprod_t, sqrt_one_minus_alphas_cumprod_t; step_noise / q_noise [S, B,4,H,W].  Returns (x, x_inter): the
        final latent and the [len(log_steps), B,4,H,W] logged latents (None without log steps).  x_T is not modified."""
        S = len(timesteps)
        return self._device_loop('sample_ancestral', _lib.FgdmAncestralParams(), x_T, cond, None, out, 'S', S,
                                 dict({'timesteps': (timesteps, C.c_int64, S)},
                                      **{k: tables.get(k) for k in ('sqrt_recip_alphas_cumprod', 'sqrt_recipm1_alphas_cumprod',
                                                                    'posterior_mean_coef1', 'posterior_mean_coef2', 'std',
                                                                    'sqrt_alphas_cumprod_t', 'sqrt_one_minus_alphas_cumprod_t')}),
                                 dict(step_noise=(step_noise, (S,)), q_noise=(q_noise, (S,)), mask=(mask, ()), x0=(x0, ())),
                                 (log_steps, dict(x_inter_out=x_inter_out)), control_scales, flags=int(flags))

    def ddim_encode(self, x0, cond, uncond, cfg_scale, timesteps, cx, ce, log_steps=(), control_scales=None, flags=0, out=None,
                    x_inter_out=None):
        """DDIM inversion on the device (fgdm_ddim_encode, include/fgdm.h): S = len(timesteps) steps over ascending timesteps
        with the per-step coefficients cx / ce (fgdm_amd.samplers.encode_tables).  Returns (x, x_inter) as sample_ancestral;
        x0 is not modified."""
        S = len(timesteps)
        return self._device_loop('ddim_encode', _lib.FgdmDdimEncodeParams(), x0, cond, uncond, out, 'S', S,
                                 dict(timesteps=(timesteps, C.c_int64, S), cx=cx, ce=ce), logs=(log_steps, dict(x_inter_out=x_inter_out)),
                                 control_scales=control_scales, cfg_scale=float(cfg_scale), flags=int(flags))


# ---------------------------------------------------------------------- fused sampler updates
def ddim_step(x, e_cond, e_uncond, cfg_scale, a_t, a_prev, sigma_t, sqrt_one_minus_at, noise=None,
              want_pred_x0=True):
    lib = _lib.load()
    x_prev = torch.empty_like(x)
    pred = torch.empty_like(x) if want_pred_x0 else None
    rc = lib.fgdm_ddim_step(_ptr(x), _ptr(e_cond), _ptr(e_uncond), float(cfg_scale), float(a_t), float(a_prev),
                            float(sigma_t), float(sqrt_one_minus_at), _ptr(noise), _ptr(x_prev), _ptr(pred),
                            C.c_void_p(0), x.numel(), _stream())
    if rc != 0:
        raise RuntimeError(f'fgdm_ddim_step failed: {rc}')
    return x_prev, pred


def posterior_sample(moments, noise=None, scale=1.0):
    """z = scale * (mean + exp(0.5 * clamp(logvar, -30, 20)) * noise) from moments [B, 2*zc, ...] = mean | logvar (device, fp32);
    noise None: scale * mean (the distribution's mode)."""
    lib = _lib.load()
    moments = moments.to(torch.float32).contiguous()
    B, c2 = moments.shape[:2]
    if c2 % 2:
        raise ValueError(f'posterior_sample: moments {tuple(moments.shape)} must hold mean | logvar along dim 1')
    z = torch.empty((B, c2 // 2, *moments.shape[2:]), device=moments.device, dtype=torch.float32)
    if noise is not None:
        noise = noise.to(torch.float32).contiguous()
        if tuple(noise.shape) != tuple(z.shape):
            raise ValueError(f'posterior_sample: noise {tuple(noise.shape)} must have the shape of the mean {tuple(z.shape)}')
    rc = lib.fgdm_posterior_sample(_ptr(moments), _ptr(noise), float(scale), _ptr(z), B, c2 // 2, z[0, 0].numel(), _stream())
    if rc != 0:
        raise RuntimeError(f'fgdm_posterior_sample failed: {rc}')
    return z


def _weights(w_pix, w_tie, device, grid=None):
    """the blending tables as contiguous fp32 on `device`; grid = (H, W, ks, stride, f): their sizes must match the crops the
    native call will read them for (a grid the crops do not cover is left to the library to refuse)"""
    w_pix, w_tie = w_pix.to(device, torch.float32).contiguous(), w_tie.to(device, torch.float32).contiguous()
    if grid is not None:
        H, W, (kh, kw), (sh, sw), f = grid
        if tuple(w_pix.shape) != (kh * f, kw * f):
            raise ValueError(f'w_pix {tuple(w_pix.shape)} must be {(kh * f, kw * f)}')
        if min(sh, sw) >= 1 and kh <= H and kw <= W and w_tie.numel() < ((H - kh) // sh + 1) * ((W - kw) // sw + 1):
            raise ValueError(f'w_tie has {w_tie.numel()} entries, fewer than the crops of the grid')
    return w_pix, w_tie


def unfold(x, ks, stride, l0=0, n=None, out=None):
    """torch.nn.Unfold(ks, stride=stride) of x fp32 [B,C,H,W] (device), crops [l0, l0 + n) (default: all from l0) as fp32
    [n,B,C,kh,kw]: crop l = ly * Lx + lx starts at (ly * stride[0], lx * stride[1])."""
    lib = _lib.load()
    x = x.to(torch.float32).contiguous()
    B, Cc, H, W = x.shape
    (kh, kw), (sh, sw) = ks, stride
    if kh > H or kw > W or min(kh, kw, sh, sw) < 1:
        raise ValueError(f'unfold: crop {tuple(ks)} / stride {tuple(stride)} do not fit {H} x {W}')
    L = ((H - kh) // sh + 1) * ((W - kw) // sw + 1)
    n = L - l0 if n is None else n
    crops = torch.empty(n, B, Cc, kh, kw, device=x.device, dtype=torch.float32) if out is None else out
    rc = lib.fgdm_unfold(_ptr(x), B, Cc, H, W, kh, kw, sh, sw, int(l0), int(n), _ptr(crops), _stream())
    if rc != 0:
        raise RuntimeError(f'fgdm_unfold failed: {rc}')
    return crops


def fold_weighted(crops, w_pix, w_tie, size, stride, crops_per_pass=0, out=None):
    """fold(crops * weighting) / fold(weighting): crops fp32 [L,B,C,kh,kw] (device) of ALL crops -> fp32 [B,C,*size];
    w_pix [kh,kw], w_tie [L] as fgdm_amd.patches.weights returns them."""
    lib = _lib.load()
    crops = crops.to(torch.float32).contiguous()
    L, B, Cc, kh, kw = crops.shape
    w_pix, w_tie = _weights(w_pix, w_tie, crops.device)
    if tuple(w_pix.shape) != (kh, kw) or w_tie.numel() != L:
        raise ValueError(f'fold_weighted: weights {tuple(w_pix.shape)}, {tuple(w_tie.shape)} do not match crops {tuple(crops.shape)}')
    Ho, Wo = size
    if kh > Ho or kw > Wo or min(stride) < 1 or L != ((Ho - kh) // stride[0] + 1) * ((Wo - kw) // stride[1] + 1):
        raise ValueError(f'fold_weighted: {L} crops of {kh} x {kw} every {tuple(stride)} do not make a {Ho} x {Wo} grid')
    y = torch.empty(B, Cc, Ho, Wo, device=crops.device, dtype=torch.float32) if out is None else out
    rc = lib.fgdm_fold_weighted(_ptr(crops), _ptr(w_pix), _ptr(w_tie), B, Cc, Ho, Wo, kh, kw, stride[0], stride[1],
                                int(crops_per_pass), _ptr(y), _stream())
    if rc != 0:
        raise RuntimeError(f'fgdm_fold_weighted failed: {rc}')
    return y


def cfg_combine(e_cond, e_uncond, cfg_scale):
    """e_u + s (e_c - e_u) as its own launch (used by PLMS, which needs e_t before the update)."""
    lib = _lib.load()
    e = torch.empty_like(e_cond)
    rc = lib.fgdm_ddim_step(_ptr(e_cond), _ptr(e_cond), _ptr(e_uncond), float(cfg_scale), 1.0, 1.0, 0.0, 0.0,
                            C.c_void_p(0), C.c_void_p(0), C.c_void_p(0), _ptr(e), e.numel(), _stream())
    if rc != 0:
        raise RuntimeError(f'fgdm_ddim_step(cfg) failed: {rc}')
    return e


def plms_combine(e_t, old_eps):
    lib = _lib.load()
    order = len(old_eps)
    out = torch.empty_like(e_t)
    e1 = old_eps[-1]
    e2 = old_eps[-2] if order >= 2 else None
    e3 = old_eps[-3] if order >= 3 else None
    rc = lib.fgdm_plms_combine(_ptr(e_t), _ptr(e1), _ptr(e2), _ptr(e3), min(order, 3), _ptr(out), e_t.numel(), _stream())
    if rc != 0:
        raise RuntimeError(f'fgdm_plms_combine failed: {rc}')
    return out


def axpby(a, ca, b, cb):
    lib = _lib.load()
    y = torch.empty_like(a)
    rc = lib.fgdm_axpby(_ptr(a), float(ca), _ptr(b), float(cb), _ptr(y), a.numel(), _stream())
    if rc != 0:
        raise RuntimeError(f'fgdm_axpby failed: {rc}')
    return y


def dpm_program_step(x_eval, e_cond, e_uncond, cfg_scale, conv_x, conv_e, base, hist, slot, planes, coefs):
    """One record of a DPM-Solver program behind its network evaluation (fgdm_op_dpm_program_step, include/fgdm.h): the model value
    goes to hist[slot] in place (slot -1: nowhere), the update's result is returned.  hist: the three history planes (None: absent)."""
    lib = _lib.load()
    n = len(planes)
    out = torch.empty_like(base)
    src, cf = (C.c_int32 * n)(*[int(v) for v in planes]), (C.c_float * n)(*[float(v) for v in coefs])
    rc = lib.fgdm_op_dpm_program_step(_ptr(x_eval), _ptr(e_cond), _ptr(e_uncond), float(cfg_scale), float(conv_x), float(conv_e),
                                      _ptr(base), _ptr(hist[0]), _ptr(hist[1]), _ptr(hist[2]), int(slot), n,
                                      C.cast(src, C.c_void_p), C.cast(cf, C.c_void_p), _ptr(out), C.c_void_p(0), C.c_void_p(0),
                                      base.numel(), _stream())
    if rc != 0:
        raise RuntimeError(f'fgdm_op_dpm_program_step failed: {rc}')
    return out


def mask_blend(a, b, mask):
    """a*mask + (1-mask)*b with a full-shape mask."""
    lib = _lib.load()
    y = torch.empty_like(a)
    rc = lib.fgdm_mask_blend(_ptr(a), _ptr(b), _ptr(mask), _ptr(y), a.numel(), _stream())
    if rc != 0:
        raise RuntimeError(f'fgdm_mask_blend failed: {rc}')
    return y


def ancestral_step(x, eps, sqrt_recip, sqrt_recipm1, coef1, coef2, std, noise=None):
    lib = _lib.load()
    out = torch.empty_like(x)
    rc = lib.fgdm_ancestral_step(_ptr(x), _ptr(eps), float(sqrt_recip), float(sqrt_recipm1), float(coef1),
                                 float(coef2), float(std), _ptr(noise), _ptr(out), x.numel(), _stream())
    if rc != 0:
        raise RuntimeError(f'fgdm_ancestral_step failed: {rc}')
    return out
