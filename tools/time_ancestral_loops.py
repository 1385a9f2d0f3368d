"""Same-process A/B of the per-step route against the device route for the ancestral sampler (LatentDiffusion.p_sample_loop,
timesteps=200) and for DDIM inversion (ControlDDIMSampler.encode, t_enc = 50 of a 50-step schedule, CFG 7.5): the SD-v1 UNet with
synthetic weights, 64 x 64 latents, B = 16 and B = 1.  Per case one warm-up of each route, then the routes alternate, `--runs`
timed runs each (host clock around a run that ends in a device synchronise, the generator re-seeded in front of every run);
prints the median per route, every sample, and whether the two routes gave the same bits.

    python tools/time_ancestral_loops.py [--runs 3] [--out profiles/ancestral_loop_timing.json]

FGDM_LIB selects another build of the library (fgdm_amd/_lib.py)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from fgdm_amd import models, samplers, synth
    from fgdm_amd.engine import SD_V1, Engine
    e = Engine(SD_V1)
    for k, shape in e.param_shapes().items():
        e.load_tensor(k, synth.make_tensor(k, shape))
    e.finalize()
    ldm = {loop: models.LatentDiffusion(SD_V1, engine=e, use_adapter=False, device_loop=loop) for loop in (False, True)}
    enc = {loop: samplers.ControlDDIMSampler(ldm[False], device_loop=loop) for loop in (False, True)}
    for s in enc.values():
        s.make_schedule(50, verbose=False)
    rows = []
    for name, steps in (('ancestral', 200), ('encode', 50)):
        for B in (16, 1):
            x = torch.from_numpy(synth.latents(B, 64, 64, seed=42)).cuda()
            c = torch.from_numpy(synth.context(B, seed=43)).cuda()
            uc = torch.from_numpy(synth.context(B, seed=44)).cuda()

            def run(loop):
                torch.manual_seed(7)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if name == 'ancestral':
                    out = ldm[loop].p_sample_loop(c, (B, 4, 64, 64), x_T=x, timesteps=steps)
                else:
                    out = enc[loop].encode(x, c, steps, unconditional_guidance_scale=7.5, unconditional_conditioning=uc)[0]
                torch.cuda.synchronize()
                return time.perf_counter() - t0, out
            outs = {loop: run(loop)[1] for loop in (False, True)}          # warm-up, and the bits
            times = {False: [], True: []}
            for _ in range(a.runs):
                for loop in (False, True):
                    times[loop].append(run(loop)[0])
            row = dict(sampling=name, steps=steps, B=B, same_bits=bool(torch.equal(outs[False], outs[True])),
                       per_step_s=statistics.median(times[False]), device_loop_s=statistics.median(times[True]),
                       per_step_samples=times[False], device_loop_samples=times[True])
            row['device_loop_over_per_step'] = row['device_loop_s'] / row['per_step_s']
            rows.append(row)
            print(json.dumps(row), flush=True)
    e.close()
    res = dict(device=torch.cuda.get_device_name(0), runs=a.runs, latent=[64, 64], network='SD-v1 UNet, no ControlNet', cases=rows)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
