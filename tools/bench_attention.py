#!/usr/bin/env python3
"""Time the fused attention kernel on the shapes of the C3 workload (B = 32 rows of a CFG batch, 8 heads); TF/s are
ALGORITHMIC (4 B T Tk C).  Usage (GPU box): python tools/bench_attention.py [--iters 20] [--long]
--long: the text-attention shapes at two and three 77-token parts (154 / 231 keys) with the 77-key shape as the control; run it
once per setting of FGDM_ATTN_CROSS_LONG (0 = the general kernel, the dispatch of before) for a same-box A/B.
--d64: head width 64 (SD-2.x networks: 5 / 10 heads) next to the d = 40 / 80 shapes of the same T; run it once more under
FGDM_ATTN_DQ80=0 for two-strand against ping-pong (profiles/attention_d64.txt).
--capture: the text shapes (Tk = 77) three ways: the product kernel, its capturing instantiation (cross-attention maps: per-head
planes written), and that plus the head reduction (profiles/attention_capture_cost.txt)."""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fgdm_amd import _lib

SHAPES = [(32, 8, 4096, 4096, 40), (32, 8, 4096, 77, 40), (32, 8, 1024, 1024, 80), (32, 8, 1024, 77, 80),
          (32, 8, 256, 256, 160), (32, 8, 256, 77, 160), (32, 8, 64, 64, 160), (16, 8, 4096, 4096, 40)]
# cross-attention at two / three text parts (cat(c_crossattn, 1); controlnet/cldm/hack.py: 231 tokens), 77 keys as the control
LONG_SHAPES = [(32, 8, 4096, 154, 40), (32, 8, 4096, 231, 40), (32, 8, 1024, 154, 80), (32, 8, 1024, 231, 80),
               (32, 8, 256, 154, 160), (32, 8, 256, 231, 160), (32, 8, 4096, 77, 40),
               # the other sub-tile counts of the key-resident kernel (NS = 4, 6, 7)
               (32, 8, 4096, 120, 40), (32, 8, 4096, 190, 40), (32, 8, 1024, 120, 80), (32, 8, 1024, 190, 80),
               (32, 8, 256, 120, 160), (32, 8, 256, 190, 160), (32, 8, 256, 220, 160)]
# head width 64 at the SD-2.x head counts, each followed by the SD-v1 shape of the same T (time per (batch, head) is the comparison)
D64_SHAPES = [(32, 5, 4096, 4096, 64), (32, 8, 4096, 4096, 40), (32, 10, 1024, 1024, 64), (32, 8, 1024, 1024, 80),
              (32, 5, 4096, 77, 64), (32, 8, 4096, 77, 40), (32, 10, 1024, 77, 64), (32, 8, 1024, 77, 80)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--only', type=int, default=-1, help='index into SHAPES (profiling runs)')
    ap.add_argument('--long', action='store_true', help='the long-context text-attention shapes (LONG_SHAPES)')
    ap.add_argument('--d64', action='store_true', help='head width 64 against d = 40 / 80 (D64_SHAPES)')
    ap.add_argument('--capture', action='store_true', help='Tk = 77 shapes: product kernel / capturing instantiation / + head reduction')
    a = ap.parse_args()
    lib = _lib.load()
    if a.capture:
        for B, H, T, Tk, d in [s for s in SHAPES if s[3] == 77]:
            row = []
            for call in (lambda ms: lib.fgdm_bench_attention(B, H, T, Tk, d, a.iters, ms),
                         lambda ms: lib.fgdm_bench_attention_maps(B, H, T, Tk, d, 0, a.iters, ms),
                         lambda ms: lib.fgdm_bench_attention_maps(B, H, T, Tk, d, 1, a.iters, ms)):
                ms = C.c_float()
                rc = call(C.byref(ms))
                row.append(f'{ms.value * 1e3:9.1f} us' if rc == 0 else f'rc={rc}')
            print(f'attn B{B} T{T} Tk{Tk} d{d:<4d} product {row[0]}   capturing {row[1]}   capturing + head reduction {row[2]}', flush=True)
        return
    shapes = D64_SHAPES if a.d64 else LONG_SHAPES if a.long else SHAPES
    for B, H, T, Tk, d in (shapes if a.only < 0 else [shapes[a.only]]):
        ms = C.c_float()
        rc = lib.fgdm_bench_attention(B, H, T, Tk, d, a.iters, C.byref(ms))
        fl = 4.0 * B * T * Tk * H * d
        print(f'attn B{B} T{T} Tk{Tk} d{d:<4d} rc={rc} {ms.value * 1e3:9.1f} us {fl / (ms.value * 1e-3) / 1e12:8.1f} TF/s '
              f'{ms.value * 1e3 / (B * H):8.3f} us per (batch, head)', flush=True)


if __name__ == '__main__':
    main()
