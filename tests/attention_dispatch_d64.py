"""Which attention kernel a call at head width 64 (SD-2.x networks: num_head_channels = 64) must reach: the rules of
attention_launch (fgdm_amd/csrc/attention.hip) for d = 64 stated a second time, in the order the launcher applies them, next to
tests/attention_dispatch.py (which states those of d = 40 / 80 / 160 and is older than this head width).  The ids are those of
include/fgdm.h (fgdm_debug_last_attention_kernel)."""
import os

from attention_dispatch import GENERAL, KERNEL_NAMES, LONG_TEXT, PING_PONG, TEXT_TOKEN, TWO_STRAND_32, _knob  # noqa: F401


def expected_kernel_d64(T, Tk, env=None):
    env = os.environ if env is None else env
    # 1. whole 256-query blocks, whole 64-key tiles, at least two of them: the two-strand kernel (FGDM_ATTN_DQ80, shared with d = 80)
    if _knob(env, 'FGDM_ATTN_DQ80', 1) > 0 and T % 256 == 0 and Tk % 64 == 0 and Tk >= 128:
        return TWO_STRAND_32
    # 2. every other long shape: the eight-wave ping-pong kernel
    if _knob(env, 'FGDM_ATTN_PP', 1) != 0 and T >= 256 and Tk >= 256:
        return PING_PONG
    # 3. one text part (65 - 96 keys) against at least one 128-query chunk: the key-resident kernel, three 32-key sub-tiles
    if _knob(env, 'FGDM_ATTN_CROSS', 4) > 0 and 64 < Tk <= 96 and T >= 128:
        return TEXT_TOKEN
    # 4. two or three text parts (97 - 256 keys): its NS form; every NS = 4 ... 8 fits the LDS at d = 64
    if _knob(env, 'FGDM_ATTN_CROSS_LONG', 8) > 0 and 96 < Tk <= 256 and T >= 128:
        return LONG_TEXT
    # 5. everything else
    return GENERAL


# (T, Tk, kernel the case is written for); B = 2, H = 5 in tests/test_gpu_sd21.py
D64_CASES = [
    (256, 256, TWO_STRAND_32),      # one 256-query block
    (256, 128, TWO_STRAND_32),      # ... and the smallest key count the two-strand kernel takes: two 64-key tiles, T != Tk
    (320, 320, PING_PONG),          # ragged last query block and key tile
    (256, 77, TEXT_TOKEN),          # one text part: NS = 3
    (256, 154, LONG_TEXT),          # two text parts: NS = 5
    (256, 231, LONG_TEXT),          # three text parts: NS = 8
    (64, 64, GENERAL),
]
