#!/usr/bin/env python3
"""Time the first stage on one GPU, encoder and decoder back to back in one process: AutoencoderKL.encode of 512 x 512 images
and AutoencoderKL.decode of their 64 x 64 latents at B = 1 and B = 8 (HIP events, warm, median), then one profiled encode per
batch size with the per-layer table of the engine's built-in timer (FGDM_PROF_DUMP).  Synthetic weights and images.

Usage:  python tools/bench_vae.py [--iters 30] [--out profiles/vae_encode_times.txt]
"""
import argparse
import os
import statistics
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from fgdm_amd import synth  # noqa: E402
from fgdm_amd.engine import Engine  # noqa: E402

SMALL = dict(in_channels=4, out_channels=4, model_channels=320, attention_resolutions=(1, 2), num_res_blocks=1,
             channel_mult=(1, 2), num_heads=8, context_dim=768)       # the UNet is not exercised: a small one keeps set-up short


def timed(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--res', type=int, default=512)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dump = os.path.join(tempfile.mkdtemp(), 'prof.tsv')
    os.environ['FGDM_PROF_DUMP'] = dump
    e = Engine(SMALL, vae=True, vae_encoder=True)
    for k, shape in e.param_shapes().items():
        e.load_tensor(k, synth.make_tensor(k, shape))
    e.finalize()
    lines = [f'first stage at {a.res} x {a.res}, {torch.cuda.get_device_name(0)}, one process, HIP events, warm, median of {a.iters} (min .. max), ms']
    tables = []
    for B in (1, 8):
        img = torch.from_numpy(synth.image(B, res=a.res, seed=a.res)).cuda()
        z = e.posterior_sample(e.vae_encode(img), None, 0.18215)
        enc = timed(lambda: e.vae_encode(img), a.iters)
        dec = timed(lambda: e.vae_decode(z, 1.0 / 0.18215), a.iters)
        enc2 = timed(lambda: e.vae_encode(img), a.iters)           # again after the decoder: the order must not matter
        lines.append(f'B={B}  vae_encode {enc[0]:8.3f} ({enc[1]:.3f} .. {enc[2]:.3f})   vae_decode {dec[0]:8.3f} ({dec[1]:.3f} .. {dec[2]:.3f})   '
                     f'vae_encode again {enc2[0]:8.3f}   per image: encode {min(enc[0], enc2[0]) / B:.3f}  decode {dec[0] / B:.3f}  '
                     f'encode / decode {min(enc[0], enc2[0]) / dec[0]:.3f}')
        e.profile_begin(1)
        e.vae_encode(img)
        tot = e.profile_end()
        rows = [l.rstrip('\n').split('\t') for l in open(dump)]
        rows.sort(key=lambda r: -float(r[2]))
        tables.append(f'\nprofiled vae_encode, B={B} (every launch bracketed; classes: ' +
                      ', '.join(f'{k} {v["ms"]:.3f} ms / {v["launches"]} launches' for k, v in tot.items()) + ')\n' +
                      f'{"ms":>9s} {"launches":>8s} {"TFLOP/s":>8s}  tag\n' +
                      '\n'.join(f'{float(r[2]):9.4f} {int(float(r[1])):8d} {(float(r[3]) / float(r[2]) / 1e9 if r[0].startswith("igemm") and float(r[2]) > 0 else 0):8.1f}  {r[0]}'
                                for r in rows))
    text = '\n'.join(lines + tables) + '\n'
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text)
    e.close()


if __name__ == '__main__':
    main()
