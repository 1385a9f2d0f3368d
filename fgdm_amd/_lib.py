"""ctypes binding of libfgdm_hip.so (the C ABI declared in include/fgdm.h).

There is deliberately NO fallback: if the shared library is missing or a symbol is
absent, importing the product path fails loudly."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, 'libfgdm_hip.so')

MAX_LEVELS = 8
MAX_CONTROLNETS = 4

FLAG_USE_ORIGINAL = 1
FLAG_ONLY_MID_CONTROL = 2
FLAG_NO_CONTROL = 4
FLAG_CFG_PAIRS = 8

ACT_NONE, ACT_SILU, ACT_RELU, ACT_GEGLU, ACT_QGELU = 0, 1, 2, 3, 4
OUT_F16, OUT_F32, OUT_F32_NCHW, OUT_F16_T = 0, 1, 2, 3
STRIDE2_PAD_BR = -2     # fgdm_op_conv2d `stride`: stride 2, zero padding bottom / right only (the first-stage encoder's Downsample)


class FgdmConfig(C.Structure):
    _fields_ = [
        ('in_channels', C.c_int32), ('out_channels', C.c_int32), ('model_channels', C.c_int32),
        ('num_res_blocks', C.c_int32), ('n_levels', C.c_int32), ('channel_mult', C.c_int32 * MAX_LEVELS),
        ('n_attention_resolutions', C.c_int32), ('attention_resolutions', C.c_int32 * MAX_LEVELS),
        ('num_heads', C.c_int32), ('context_dim', C.c_int32), ('use_adapter', C.c_int32),
        ('n_controlnets', C.c_int32), ('hint_channels', C.c_int32), ('workspace_bytes', C.c_int64),
        ('vae_ch', C.c_int32), ('vae_n_levels', C.c_int32), ('vae_ch_mult', C.c_int32 * MAX_LEVELS),
        ('vae_num_res_blocks', C.c_int32), ('vae_z_channels', C.c_int32), ('vae_out_ch', C.c_int32),
        ('clip_layers', C.c_int32), ('clip_width', C.c_int32), ('clip_heads', C.c_int32), ('clip_mlp', C.c_int32),
        ('clip_vocab', C.c_int32), ('clip_max_len', C.c_int32),
        ('n_extra_adapters', C.c_int32),
        ('vae_encoder', C.c_int32),
    ]


class FgdmConfig2(FgdmConfig):
    """fgdm_config as include/fgdm.h declares it today: the 208-byte struct above (whose last four bytes, `reserved0` in the
    header, were its tail padding) followed by the SD-2.x fields.  A ctypes subclass lays its own fields out after the WHOLE base,
    padding included, which is exactly where the header puts them (offsets 208 and 212); zero in both means the networks the
    208-byte struct described."""
    _fields_ = [('num_head_channels', C.c_int32), ('use_linear_in_transformer', C.c_int32)]


class FgdmDdimParams(C.Structure):
    """fgdm_ddim_params of include/fgdm.h (fgdm_sample_ddim_ex); struct_size must be ctypes.sizeof of this class."""
    _fields_ = [('struct_size', C.c_int64)] + [(name, C.c_void_p) for name in (
        'x', 'cond', 'uncond', 'timesteps', 'alphas', 'alphas_prev', 'sqrt_one_minus_alphas', 'control_scales', 'sigmas',
        'cfg_scales', 'step_noise', 'mask', 'x0', 'q_noise', 'sqrt_alphas_cumprod_t', 'sqrt_one_minus_alphas_cumprod_t',
        'log_steps', 'x_inter_out', 'pred_x0_out')] + [('cfg_scale', C.c_float)] + [(name, C.c_int32) for name in (
            'S', 'B', 'H', 'W', 'flags', 'n_log', 'reserved0')]


class FgdmPlmsParams(C.Structure):
    """fgdm_plms_params of include/fgdm.h (fgdm_sample_plms); struct_size must be ctypes.sizeof of this class."""
    _fields_ = [('struct_size', C.c_int64)] + [(name, C.c_void_p) for name in (
        'x', 'cond', 'uncond', 'timesteps', 'alphas', 'alphas_prev', 'sqrt_one_minus_alphas', 'control_scales', 'mask', 'x0',
        'q_noise', 'sqrt_alphas_cumprod_t', 'sqrt_one_minus_alphas_cumprod_t', 'log_steps', 'x_inter_out', 'pred_x0_out')] + [
            ('cfg_scale', C.c_float)] + [(name, C.c_int32) for name in ('S', 'B', 'H', 'W', 'flags', 'n_log', 'reserved0')]


class FgdmDpmppParams(C.Structure):
    """fgdm_dpmpp_params of include/fgdm.h (fgdm_sample_dpmpp); struct_size must be ctypes.sizeof of this class."""
    _fields_ = [('struct_size', C.c_int64)] + [(name, C.c_void_p) for name in (
        'x', 'cond', 'uncond', 'control_scales', 't_float', 'inv_alpha', 'neg_sigma_over_alpha', 'update_kind', 'c1', 'cm0',
        'cm1')] + [('cfg_scale', C.c_float)] + [(name, C.c_int32) for name in (
            'n_eval', 'B', 'H', 'W', 'flags', 'reserved0', 'reserved1')]


class FgdmDpmSolverParams(C.Structure):
    """fgdm_dpm_solver_params of include/fgdm.h (fgdm_sample_dpm_solver); struct_size must be ctypes.sizeof of this class."""
    _fields_ = [('struct_size', C.c_int64)] + [(name, C.c_void_p) for name in (
        'x', 'cond', 'uncond', 'control_scales', 't_float', 'conv_x', 'conv_e', 'slot', 'nterms', 'plane', 'coef', 'dest')] + [
            ('cfg_scale', C.c_float)] + [(name, C.c_int32) for name in ('n_eval', 'B', 'H', 'W', 'flags', 'reserved0', 'reserved1')]


class FgdmAncestralParams(C.Structure):
    """fgdm_ancestral_params of include/fgdm.h (fgdm_sample_ancestral); struct_size must be ctypes.sizeof of this class."""
    _fields_ = [('struct_size', C.c_int64)] + [(name, C.c_void_p) for name in (
        'x', 'cond', 'timesteps', 'sqrt_recip_alphas_cumprod', 'sqrt_recipm1_alphas_cumprod', 'posterior_mean_coef1',
        'posterior_mean_coef2', 'std', 'step_noise', 'control_scales', 'mask', 'x0', 'q_noise', 'sqrt_alphas_cumprod_t',
        'sqrt_one_minus_alphas_cumprod_t', 'log_steps', 'x_inter_out')] + [(name, C.c_int32) for name in (
            'S', 'B', 'H', 'W', 'flags', 'n_log', 'reserved0', 'reserved1')]


class FgdmDdimEncodeParams(C.Structure):
    """fgdm_ddim_encode_params of include/fgdm.h (fgdm_ddim_encode); struct_size must be ctypes.sizeof of this class."""
    _fields_ = [('struct_size', C.c_int64)] + [(name, C.c_void_p) for name in (
        'x', 'cond', 'uncond', 'timesteps', 'cx', 'ce', 'control_scales', 'log_steps', 'x_inter_out')] + [
            ('cfg_scale', C.c_float)] + [(name, C.c_int32) for name in ('S', 'B', 'H', 'W', 'flags', 'n_log', 'reserved0')]


class FgdmAttentionCapture(C.Structure):
    """fgdm_attention_capture of include/fgdm.h (fgdm_attention_capture_set); struct_size must be ctypes.sizeof of this class."""
    _fields_ = [('struct_size', C.c_int64), ('tokens', C.POINTER(C.c_int32)), ('block_mask', C.c_uint32)] + [
        (name, C.c_int32) for name in ('n_tokens', 'rows', 'mode', 'batch', 'latent_h', 'latent_w', 'reserved0')]


class FgdmNoisePlan(C.Structure):
    """fgdm_noise_plan of include/fgdm.h (fgdm_loop_noise_set); struct_size must be ctypes.sizeof of this class."""
    _fields_ = [('struct_size', C.c_int64), ('seed', C.c_uint64), ('first_sample', C.c_int32), ('first_step', C.c_int32),
                ('temperature', C.c_float), ('repeat_noise', C.c_int32), ('reserved0', C.c_int32), ('reserved1', C.c_int32)]


NOISE_STREAM_STEP, NOISE_STREAM_Q = 0, 1      # the generator's stream ids: the sampler's step noise, q_sample's noise
ATTENTION_CAPTURE_MAX_KEYS = 256                                        # FGDM_ATTENTION_CAPTURE_MAX_KEYS
CAPTURE_ROWS = {'all': 0, 'cond': 1, 'uncond': 2}                       # FGDM_CAPTURE_ROWS_*
CAPTURE_MODES = {'sum': 0, 'last': 1}                                   # FGDM_CAPTURE_SUM / FGDM_CAPTURE_LAST
DPMPP_FIRST, DPMPP_SECOND = 1, 2      # FGDM_DPMPP_FIRST / FGDM_DPMPP_SECOND
DPM_PLANE_BASE, DPM_PLANE_HIST0, DPM_PLANE_M, DPM_DEST_STATE, DPM_DEST_EVAL = 0, 1, 4, 1, 2      # FGDM_DPM_PLANE_* / FGDM_DPM_DEST_*
PLMS_PROBE, PLMS_FINISH_FIRST, PLMS_MULTISTEP = 0, 1, 2      # the modes of fgdm_op_plms_loop_step

_p = C.c_void_p
_f = C.c_float
_i = C.c_int
_i64 = C.c_int64

# name -> (restype, argtypes); every symbol include/fgdm.h declares
SIGNATURES = {
    'fgdm_create': (_i, [C.POINTER(FgdmConfig), _i, C.POINTER(_p)]),
    'fgdm_destroy': (None, [_p]),
    'fgdm_last_error': (C.c_char_p, [_p]),
    'fgdm_param_count': (_i, [C.POINTER(FgdmConfig)]),
    'fgdm_param_info': (_i, [C.POINTER(FgdmConfig), _i, C.c_char_p, _i, C.POINTER(_i64), C.POINTER(_i)]),
    'fgdm_load_tensor': (_i, [_p, C.c_char_p, _p, _i, C.POINTER(_i64), _i]),
    'fgdm_finalize_weights': (_i, [_p]),
    'fgdm_set_hint': (_i, [_p, _i, _p, _i, _i, _i, _p]),
    'fgdm_set_concat': (_i, [_p, _p, _i, _i, _i, _i, _p]),
    'fgdm_set_adapter_conds': (_i, [_p, _p, _i, _i, _i, _i, _p]),
    'fgdm_set_context': (_i, [_p, _p, _i, _p]),
    'fgdm_apply_model': (_i, [_p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _p, _p]),
    'fgdm_clip_encode': (_i, [_p, _p, _i, _i, _p, _p]),
    'fgdm_clip_encode_skip': (_i, [_p, _p, _i, _i, _i, _p, _p]),
    'fgdm_set_context_tokens': (_i, [_p, _i]),
    'fgdm_get_context_tokens': (_i, [_p]),
    'fgdm_attention_capture_set': (_i, [_p, C.POINTER(FgdmAttentionCapture)]),
    'fgdm_attention_capture_reset': (_i, [_p, _p]),
    'fgdm_attention_capture_info': (_i, [_p, _i, C.POINTER(_i64), C.POINTER(C.c_int32)]),
    'fgdm_attention_capture_block_size': (_i, [_p, _i, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    'fgdm_attention_capture_read': (_i, [_p, _i, _p, _p]),
    'fgdm_run_block': (_i, [_p, C.c_char_p, _p, _i, _p, _i, _p, _p, _i, _i, _i, _p, _i64, C.POINTER(_i64), _p]),
    'fgdm_vae_decode': (_i, [_p, _p, _i, _i, _i, _f, _p, _p]),
    'fgdm_vae_encode': (_i, [_p, _p, _i, _i, _i, _p, _p]),
    'fgdm_unfold': (_i, [_p] + [_i] * 10 + [_p, _p]),
    'fgdm_fold_weighted': (_i, [_p, _p, _p] + [_i] * 9 + [_p, _p]),
    'fgdm_vae_decode_patches': (_i, [_p, _p, _i, _i, _i, _f] + [_i] * 5 + [_p, _p, _i, _p, _p]),
    'fgdm_apply_model_patches': (_i, [_p, _p, _p, _p, _p] + [_i] * 7 + [_p, _p, _i, _i, _p, _p]),
    'fgdm_posterior_sample': (_i, [_p, _p, _f, _p, _i, _i, _i, _p]),
    'fgdm_image_to_uint8': (_i, [_p, _i, _i, _i, _i, _i, _p, _p]),
    'fgdm_resize_linear_uint8': (_i, [_p, _i, _i, _i, _i, _i, _i, _p, _p]),
    'fgdm_uint8_to_hint': (_i, [_p, _i, _i, _i, _i, _p, _p]),
    'fgdm_controlnet': (_i, [_p, _i, _p, _p, _p, _i, _i, _i, _p, _i64, _p]),
    'fgdm_ddim_step': (_i, [_p, _p, _p, _f, _f, _f, _f, _f, _p, _p, _p, _p, _i64, _p]),
    'fgdm_plms_combine': (_i, [_p, _p, _p, _p, _i, _p, _i64, _p]),
    'fgdm_axpby': (_i, [_p, _f, _p, _f, _p, _i64, _p]),
    'fgdm_mask_blend': (_i, [_p, _p, _p, _p, _i64, _p]),
    'fgdm_ancestral_step': (_i, [_p, _p, _f, _f, _f, _f, _f, _p, _p, _i64, _p]),
    'fgdm_sample_ddim': (_i, [_p, _p, _p, _p, _f, _i, C.POINTER(_i64), C.POINTER(_f), C.POINTER(_f), C.POINTER(_f),
                              _p, _i, _i, _i, _i, _p]),
    'fgdm_sample_ddim_ex': (_i, [_p, C.POINTER(FgdmDdimParams), _p]),
    'fgdm_op_ddim_loop_step': (_i, [_p, _p, _p, _f, _f, _f, _f, _f, _p, _p, _p, _p, _f, _f, _p, _p, _p, _p, _p, _i64, _p]),
    'fgdm_sample_plms': (_i, [_p, C.POINTER(FgdmPlmsParams), _p]),
    'fgdm_sample_dpmpp': (_i, [_p, C.POINTER(FgdmDpmppParams), _p]),
    'fgdm_op_plms_loop_step': (_i, [_p, _p, _p, _f, _i, _i, _p, _p, _p, _p, _f, _f, _f, _p, _p, _p, _f, _f, _p, _p, _p, _p, _p,
                                    _i64, _p]),
    'fgdm_op_dpmpp_loop_step': (_i, [_p, _p, _p, _f, _f, _f, _p, _i, _f, _f, _f, _p, _p, _p, _p, _i64, _p]),
    'fgdm_sample_dpm_solver': (_i, [_p, C.POINTER(FgdmDpmSolverParams), _p]),
    'fgdm_op_dpm_program_step': (_i, [_p, _p, _p, _f, _f, _f, _p, _p, _p, _p, _i, _i, _p, _p, _p, _p, _p, _i64, _p]),
    'fgdm_sample_ancestral': (_i, [_p, C.POINTER(FgdmAncestralParams), _p]),
    'fgdm_ddim_encode': (_i, [_p, C.POINTER(FgdmDdimEncodeParams), _p]),
    'fgdm_loop_noise_set': (_i, [_p, C.POINTER(FgdmNoisePlan)]),
    'fgdm_randn': (_i, [C.c_uint64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _f, _p, C.c_int32, C.c_int32, _p]),
    'fgdm_op_rand_bits': (_i, [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _p, _i64, _p]),
    'fgdm_op_ancestral_loop_step': (_i, [_p, _p, _f, _f, _f, _f, _f, _p, _p, _p, _p, _f, _f, _p, _p, _p, _i64, _p]),
    'fgdm_op_invert_loop_step': (_i, [_p, _p, _p, _f, _f, _f, _p, _p, _p, _p, _i64, _p]),
    'fgdm_profile_begin': (_i, [_p, _i]),
    'fgdm_profile_end': (_i, [_p, C.POINTER(C.c_double)]),
    'fgdm_workspace_stats': (_i, [_p, C.POINTER(_i64), C.POINTER(_i64)]),
    'fgdm_launch_stats': (_i, [_p, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64)]),
    'fgdm_replay_plan': (_i, [_i, _p, _p, _p, _p, _i, _i, _p, _i, _p]),
    'fgdm_op_conv2d': (_i, [_p, _i, _p, _i, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _f, _p, _p]),
    'fgdm_op_linear': (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _p, _p]),
    'fgdm_debug_force_igemm_cfg': (_i, [_i]),
    'fgdm_bench_igemm': (_i, [_i] * 13 + [C.POINTER(_f)]),
    'fgdm_op_linear_ln_linear': (_i, [_p] * 8 + [_i] * 5 + [_p, _p, C.POINTER(_i), _p]),
    'fgdm_bench_norm': (_i, [_i] * 7 + [C.POINTER(_f)]),
    'fgdm_bench_attention': (_i, [_i] * 6 + [C.POINTER(_f)]),
    'fgdm_bench_attention_maps': (_i, [_i] * 7 + [C.POINTER(_f)]),
    'fgdm_bench_ff': (_i, [_i] * 4 + [C.POINTER(_f)]),
    'fgdm_op_groupnorm': (_i, [_p, _i, _p, _i, _i, _i, _p, _p, _f, _i, _p, _p]),
    'fgdm_op_layernorm': (_i, [_p, _i, _i, _p, _p, _f, _p, _p]),
    'fgdm_op_attention': (_i, [_p, _i, _p, _i, _p, _i, _p, _i, _i, _i, _i, _i, _i, _p]),
    'fgdm_op_attention_ex': (_i, [_p, _i, _p, _i, _p, _i, _p, _i, _i, _i, _i, _i, _i, _i, _p]),
    'fgdm_debug_last_attention_kernel': (_i, []),
    'fgdm_op_cross_attention_maps': (_i, [_p, _i, _p, _i, _p, _i, _p, _i, _p, _i, _i, _i, _i, _i, _i, _p]),
    'fgdm_op_small_attention': (_i, [_p, _i, _i, _i, _p, _i, _i, _i, _i, _i, _i, _p]),
    'fgdm_op_vae_attention': (_i, [_p, _p, _p, _p, _i, _i, _i, _p]),
    'fgdm_op_softmax_rows': (_i, [_p, _p, _i, _i, _p]),
    'fgdm_op_nchw_to_nhwc': (_i, [_p, _p, _i, _i, _i, _i, _p]),
    'fgdm_op_nhwc_to_nchw': (_i, [_p, _p, _i, _i, _i, _p]),
    'fgdm_op_pack_xcat': (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _p, _p]),
    'fgdm_op_avgpool2': (_i, [_p, _p, _i, _i, _i, _i, _p]),
    'fgdm_op_transpose_pad': (_i, [_p, _p, _i, _i, _i, _i, _p]),
    'fgdm_op_timestep_embed': (_i, [_p, _p, _p, _i, _i, _i, _p]),
    'fgdm_op_add_f16': (_i, [_p, _p, _p, _i64, _p]),
    'fgdm_op_embed_tokens': (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _p]),
    'fgdm_op_layernorm32': (_i, [_p, _i, _i, _p, _p, _f, _p, _p, _p]),
    'fgdm_op_add_f16_to_f32': (_i, [_p, _p, _p, _i64, _p]),
    'fgdm_op_f32_to_f16': (_i, [_p, _p, _i64, _p]),
    'fgdm_op_silu_f32_to_f16': (_i, [_p, _p, _i64, _p]),
    'fgdm_op_vae_prequant': (_i, [_p, _p, _f, _p, _i, _i, _p]),
    'fgdm_op_vae_moments': (_i, [_p, _p, _p, _i, _i, _p]),
    'fgdm_op_ln_qkv': (_i, [_p] * 6 + [_i] * 5 + [_p, _p, _p]),
    'fgdm_weights_begin_update': (_i, [_p]),
    'fgdm_weights_update_tensor': (_i, [_p, C.c_char_p, _p, C.POINTER(_i64), _i]),
    'fgdm_weights_commit_update': (_i, [_p, _p]),
    'fgdm_weights_snapshot': (_i, [_p, C.POINTER(C.c_char_p), _i]),
    'fgdm_weights_restore': (_i, [_p, _p]),
    'fgdm_weights_snapshot_bytes': (_i64, [_p]),
    'fgdm_weights_update_plan': (_i, [C.POINTER(FgdmConfig), C.POINTER(C.c_char_p), _i, C.c_char_p, _i]),
    'fgdm_op_lora_merge': (_i, [_p, _p, _p, _f, _i, _i, _i, _p, _p]),
}

_lib = None


def load():
    """Load the shared library and bind every symbol.  Raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    # The library binds to whichever libamdhip64 the process already holds.  PyTorch-ROCm ships its own copy of the HIP
    # runtime: if this library were loaded first it would pull in the system copy, the process would then hold two
    # runtimes, and the second one sees "no ROCm-capable device".  Let torch (device memory / streams plumbing of the
    # Python host layer) load its runtime first.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    # FGDM_LIB: another BUILD of the same library (tools/ab_lib.sh alternates two builds on one box without touching the in-tree
    # file); it must export every symbol like the in-tree one, and there is still no fallback
    path = os.environ.get('FGDM_LIB') or LIB_PATH
    if not os.path.exists(path):
        raise RuntimeError(f'{path} not found: build it with `python -m fgdm_amd.build` '
                           '(the HIP engine is mandatory, there is no CPU fallback)')
    lib = C.CDLL(os.path.abspath(path))
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib
