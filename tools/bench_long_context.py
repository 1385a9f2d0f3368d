#!/usr/bin/env python3
"""End-to-end cost of a long text context: ms per denoising step of ControlLDM.apply_model on the C3 shape (16 prompts,
one seg-ControlNet, classifier-free guidance = 32 rows at a 64 x 64 latent) with a 77-token context against the 231-token
context of the long-prompt route (controlnet/cldm/hack.py:23-68).  Synthetic weights and inputs (fgdm_amd.synth); the
context is registered once (loop-invariant), as in a sampling loop.
Usage (GPU box): python tools/bench_long_context.py [--steps 10] [--warmup 3] [--prompts 16] [--tokens 77 231]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from fgdm_amd import _lib, synth
from fgdm_amd.engine import Engine


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--prompts', type=int, default=16)
    ap.add_argument('--tokens', type=int, nargs='+', default=[77, 231])
    ap.add_argument('--repeats', type=int, default=3)
    a = ap.parse_args()
    e = Engine(None, use_adapter=False, n_controlnets=1)
    for k, shape in e.param_shapes().items():
        e.load_tensor(k, synth.make_tensor(k, shape))
    e.finalize()
    n = a.prompts
    xs = torch.from_numpy(synth.latents(n, 64, 64, seed=1)).cuda()
    x, t = torch.cat([xs, xs]), torch.full((2 * n,), 501, dtype=torch.long).cuda()
    e.set_hint(0, torch.from_numpy(synth.hint(n, res=512, seed=3)).cuda())
    out = {'shape': f'{n} prompts x CFG = {2 * n} rows, latent 64x64, 1 ControlNet', 'steps': a.steps, 'ms_per_step': {}}
    for rep in range(a.repeats):
        for tok in a.tokens:
            ctx = torch.from_numpy(synth.context(2 * n, seed=2, tokens=tok)).cuda()
            for _ in range(a.warmup):
                e.apply_model(x, t, ctx, flags=_lib.FLAG_CFG_PAIRS)
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            ev0.record()
            for _ in range(a.steps):
                e.apply_model(x, t, ctx, flags=_lib.FLAG_CFG_PAIRS)
            ev1.record()
            torch.cuda.synchronize()
            out['ms_per_step'].setdefault(str(tok), []).append(round(ev0.elapsed_time(ev1) / a.steps, 3))
    e.close()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
