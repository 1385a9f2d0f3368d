#!/usr/bin/env python3
"""Time the patch-wise first-stage decode on one GPU (HIP events, warm, median): a 1024 x 1024 image from z [1,4,128,128] in
64 x 64 latent crops at stride 32 (9 crops of 512 x 512 pixels), next to the plain vae_decode of the same 9 crops as one batch,
and the unfold / weighted-fold kernels alone with their achieved GB/s.  Synthetic weights and latents.

Usage:  python tools/bench_patches.py [--iters 30] [--out profiles/split_input_times.txt]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from bench_vae import SMALL, timed  # noqa: E402
from fgdm_amd import engine as eng, patches, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--latent', type=int, default=128)
    ap.add_argument('--ks', type=int, default=64)
    ap.add_argument('--stride', type=int, default=32)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    e = eng.Engine(SMALL, vae=True)
    for k, shape in e.param_shapes().items():
        e.load_tensor(k, synth.make_tensor(k, shape))
    e.finalize()
    sp = dict(ks=(a.ks, a.ks), stride=(a.stride, a.stride), vqf=8, patch_distributed_vq=True, tie_braker=False,
              clip_min_weight=0.01, clip_max_weight=0.5, clip_min_tie_weight=0.01, clip_max_tie_weight=0.5)
    H = a.latent
    (kh, kw), st, Ly, Lx, f = patches.decode_geometry(H, H, sp)
    L = Ly * Lx
    w_pix, w_tie = (v.cuda() for v in patches.weights(kh * f, kw * f, Ly, Lx, sp))
    z = torch.from_numpy(synth.latents(1, H, H, seed=3000)).cuda() * 0.18215
    crops = eng.unfold(z, (kh, kw), st).reshape(L, 4, kh, kw).contiguous()
    o = e.vae_decode(crops, 1 / 0.18215).reshape(L, 1, 3, kh * f, kw * f).contiguous()
    img = torch.empty(1, 3, H * f, H * f, device='cuda')
    zc = torch.empty(L, 1, 4, kh, kw, device='cuda')
    st8 = (st[0] * f, st[1] * f)
    rows = [('patch-wise decode (unfold, decode in passes, fold)', lambda: e.vae_decode_patches(z, 1 / 0.18215, (kh, kw), st, f, w_pix, w_tie), None),
            (f'plain vae_decode of the same {L} crops as one batch', lambda: e.vae_decode(crops, 1 / 0.18215), None),
            ('... patch-wise, one crop per pass', lambda: e.vae_decode_patches(z, 1 / 0.18215, (kh, kw), st, f, w_pix, w_tie, 1), None),
            ('unfold of the latent alone', lambda: eng.unfold(z, (kh, kw), st, out=zc), 2 * zc.numel() * 4),
            ('weighted fold of the decoded crops alone (accumulate + finish)',
             lambda: eng.fold_weighted(o, w_pix, w_tie, (H * f, H * f), st8, out=img), (o.numel() + 3 * img.numel()) * 4)]
    lines = [f'split_input_params decode: z [1,4,{H},{H}] -> image {H * f} x {H * f}, crops {kh} x {kw} / stride {st[0]} (L = {L}, '
             f'{kh * f} x {kw * f} pixels each), {torch.cuda.get_device_name(0)}, HIP events, warm, median of {a.iters} (min .. max), ms']
    res = {}
    for name, fn, nbytes in rows:
        med, lo, hi = timed(fn, a.iters)
        res[name] = med
        bw = f'   {nbytes / med / 1e6:8.1f} GB/s ({nbytes / 1e6:.1f} MB: crops read or written once, image written, read and written again)' if nbytes else ''
        lines.append(f'{med:9.3f} ({lo:.3f} .. {hi:.3f})  {name}{bw}')
    names = [r[0] for r in rows]
    extra = res[names[0]] - res[names[1]]
    lines.append(f'unfold + fold (kernels alone) = {res[names[3]] + res[names[4]]:.3f} ms = '
                 f'{100 * (res[names[3]] + res[names[4]]) / res[names[1]]:.2f} % of the crops\' decode; '
                 f'patch-wise minus plain = {extra:+.3f} ms ({100 * extra / res[names[1]]:+.2f} %)')
    text = '\n'.join(lines) + '\n'
    print(text)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(text)
    e.close()


if __name__ == '__main__':
    main()
