"""Which attention kernel a call must reach: a second, independent statement of the dispatch rules of attention_launch
(fgdm_amd/csrc/attention.hip), written from its comments.  The parity tests assert fgdm_debug_last_attention_kernel() against it, so
a change to a dispatch condition that moves cases onto another kernel fails here instead of silently leaving a kernel untested.
When the two disagree, somebody has to decide which one is right.

The ids are those of include/fgdm.h (fgdm_debug_last_attention_kernel).  The knobs are read from the environment the way the
library reads them (once per process there; the tests that set them start a fresh interpreter)."""
import os

NONE, GENERAL, TEXT_TOKEN, LONG_TEXT, PING_PONG, TWO_STRAND_16, TWO_STRAND_32 = range(7)
KERNEL_NAMES = {GENERAL: 'general', TEXT_TOKEN: 'text_token', LONG_TEXT: 'long_text', PING_PONG: 'ping_pong',
                TWO_STRAND_16: 'two_strand_16', TWO_STRAND_32: 'two_strand_32'}


def _knob(env, name, default):
    v = env.get(name)
    try:
        return default if v is None else int(v)
    except ValueError:
        return 0            # atoi of a non-number


def expected_kernel(T, Tk, d, env=None):
    """kernel id for T queries, Tk keys, head width d (the tests' leading dimensions are far below the 2^31-byte tile-offset limits
    of the two-strand kernels, and their V^T rows hold at least roundup(Tk, 64) >= 96 keys wherever the text-token kernel applies)"""
    env = os.environ if env is None else env
    dq, dq80 = _knob(env, 'FGDM_ATTN_DQ', 3), _knob(env, 'FGDM_ATTN_DQ80', 1)
    pp = _knob(env, 'FGDM_ATTN_PP', 1) != 0
    cross, cross_long = _knob(env, 'FGDM_ATTN_CROSS', 4), _knob(env, 'FGDM_ATTN_CROSS_LONG', 8)
    # long attention in whole 256-query blocks and whole 64-key tiles: the two-strand kernels
    two_strand = T % 256 == 0 and Tk % 64 == 0 and Tk >= 128
    if d == 40 and dq > 0 and two_strand:
        return TWO_STRAND_16 if dq == 1 else TWO_STRAND_32
    if d == 80 and dq80 > 0 and two_strand:
        return TWO_STRAND_32
    # every other long shape at d = 40 / 80: the eight-wave ping-pong kernel
    if pp and T >= 256 and Tk >= 256 and d in (40, 80):
        return PING_PONG
    # one text part (65 - 96 keys) against at least one 128-query chunk: the key-resident kernel with three 32-key sub-tiles
    if cross > 0 and 64 < Tk <= 96 and T >= 128:
        return TEXT_TOKEN
    # two or three text parts (97 - 256 keys): the same kernel with ceil(Tk / 32) sub-tiles; d = 160 fits seven of them
    if cross_long > 0 and 96 < Tk <= 256 and T >= 128:
        ns = (Tk + 31) // 32
        if d in (40, 80) or (d == 160 and ns <= 7):
            return LONG_TEXT
    return GENERAL
