"""The kernel ids of the CAPTURING attention instantiations (fgdm_debug_last_attention_kernel): the dispatch is that of
tests/attention_dispatch.py / attention_dispatch_d64.py, and a call that those rules give to a text kernel or the general one
reports the capturing twin's id; the self-attention kernels have no capturing form (FGDM_ERR_ARG)."""
import attention_dispatch as AD
from attention_dispatch_d64 import expected_kernel_d64

GENERAL_CAP, TEXT_TOKEN_CAP, LONG_TEXT_CAP = 7, 8, 9
CAPTURING = {AD.GENERAL: GENERAL_CAP, AD.TEXT_TOKEN: TEXT_TOKEN_CAP, AD.LONG_TEXT: LONG_TEXT_CAP}
MAX_KEYS = 256


def expected_capture_kernel(T, Tk, d, env=None):
    """the id a capturing call reports, or None where it is refused"""
    if Tk > MAX_KEYS:
        return None
    plain = expected_kernel_d64(T, Tk, env) if d == 64 else AD.expected_kernel(T, Tk, d, env)
    return CAPTURING.get(plain)
