"""Same-process A/B of the per-step route against the device loop for PLMSSampler (50 steps) and DPMSolverSampler (20 steps):
the SD-v1 UNet with synthetic weights, 64 x 64 latents, CFG 7.5, B = 16 and B = 1.  (The plain UNet, not the metric's
ControlLDM: neither sampler joins the dict conditionings of a ControlLDM into one CFG batch, on either route.)
Per case one warm-up of each route, then the routes alternate, `--runs` timed samplings each (host clock around a sampling that
ends in a device synchronise); prints the median per route, every sample, and whether the two routes gave the same bits.

    python tools/time_multistep_loops.py [--runs 3] [--out profiles/multistep_loop_timing.json] [--samplers ddim,plms,dpmpp]

--samplers adds DDIMSampler (50 steps) or narrows the list; FGDM_LIB selects another build of the library (fgdm_amd/_lib.py)."""
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
    ap.add_argument('--samplers', default='plms,dpmpp', help='comma-separated: ddim (50 steps), plms (50), dpmpp (20)')
    a = ap.parse_args()
    from fgdm_amd import models, samplers, synth
    from fgdm_amd.engine import SD_V1, Engine
    e = Engine(SD_V1)
    for k, shape in e.param_shapes().items():
        e.load_tensor(k, synth.make_tensor(k, shape))
    e.finalize()
    m = models.LatentDiffusion(SD_V1, engine=e, use_adapter=False)
    rows = []
    known = dict(ddim=(samplers.DDIMSampler, 50), plms=(samplers.PLMSSampler, 50), dpmpp=(samplers.DPMSolverSampler, 20))
    for name, (cls, S) in ((k, known[k]) for k in a.samplers.split(',')):
        for B in (16, 1):
            x_T = torch.from_numpy(synth.latents(B, 64, 64, seed=42)).cuda()
            c = torch.from_numpy(synth.context(B, seed=43)).cuda()
            uc = torch.from_numpy(synth.context(B, seed=44)).cuda()
            smp = {False: cls(m), True: cls(m, device_loop=True)}

            def run(loop):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = smp[loop].sample(S, B, (4, 64, 64), c.clone(), verbose=False, x_T=x_T, unconditional_guidance_scale=7.5,
                                       unconditional_conditioning=uc.clone())[0]
                torch.cuda.synchronize()
                return time.perf_counter() - t0, out
            outs = {loop: run(loop)[1] for loop in (False, True)}          # warm-up, and the bits
            times = {False: [], True: []}
            for _ in range(a.runs):
                for loop in (False, True):
                    times[loop].append(run(loop)[0])
            row = dict(sampler=name, steps=S, B=B, same_bits=bool(torch.equal(outs[False], outs[True])),
                       per_step_s=statistics.median(times[False]), device_loop_s=statistics.median(times[True]),
                       per_step_samples=times[False], device_loop_samples=times[True])
            row['device_loop_over_per_step'] = row['device_loop_s'] / row['per_step_s']
            rows.append(row)
            print(json.dumps(row), flush=True)
    e.close()
    res = dict(device=torch.cuda.get_device_name(0), runs=a.runs, latent=[64, 64], cfg_scale=7.5, network='SD-v1 UNet, no ControlNet',
               cases=rows)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
