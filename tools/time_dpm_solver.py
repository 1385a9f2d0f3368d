"""Same-process timing of the DPM-Solver family against the existing 20-step DPM-Solver++ sampler: the SD-v1 UNet with synthetic
weights, 64 x 64 latents, CFG 7.5, B = 16 and B = 1, each configuration on the per-step route and on the device loop:

    dpmpp_20         DPMSolverSampler, 20 steps (multistep order 2, data prediction): the existing sampler
    multistep3_15    DPM_Solver(predict_x0=True).sample(steps=15, order=3, method='multistep')
    singlestep3_15   DPM_Solver(predict_x0=False).sample(steps=15, order=3, method='singlestep'): 15 network evaluations

Per case one warm-up of each route, then the routes alternate, `--runs` timed samplings each (host clock around a sampling that ends
in a device synchronise); prints the median per route, every sample, and whether the two routes gave the same bits.

    python tools/time_dpm_solver.py [--runs 3] [--out profiles/dpm_solver_timing.json]"""
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
    from fgdm_amd import dpm_solver as ds, models, samplers, synth
    from fgdm_amd.engine import SD_V1, Engine
    e = Engine(SD_V1)
    for k, shape in e.param_shapes().items():
        e.load_tensor(k, synth.make_tensor(k, shape))
    e.finalize()
    m = models.LatentDiffusion(SD_V1, engine=e, use_adapter=False)
    ns = ds.NoiseScheduleVP('discrete', alphas_cumprod=m.alphas_cumprod)
    rows, loops = [], [0]
    for entry in ('sample_dpmpp', 'sample_dpm_solver'):                # count the samplings the device loops take over
        def counted(*args, _real=getattr(e, entry), **kw):
            loops[0] += 1
            return _real(*args, **kw)
        setattr(e, entry, counted)
    for B in (16, 1):
        x_T = torch.from_numpy(synth.latents(B, 64, 64, seed=42)).cuda()
        c = torch.from_numpy(synth.context(B, seed=43)).cuda()
        uc = torch.from_numpy(synth.context(B, seed=44)).cuda()

        def old(loop):
            return samplers.DPMSolverSampler(m, device_loop=loop).sample(20, B, (4, 64, 64), c, verbose=False, x_T=x_T,
                                                                         unconditional_guidance_scale=7.5, unconditional_conditioning=uc)[0]

        def new(px0, **kw):
            def run(loop):
                fn = ds.model_wrapper(m, ns, guidance_type='classifier-free', condition=c, unconditional_condition=uc, guidance_scale=7.5)
                return ds.DPM_Solver(fn, ns, predict_x0=px0, device_loop=loop).sample(x_T, **kw)
            return run
        cases = dict(dpmpp_20=(old, 20), multistep3_15=(new(True, steps=15, order=3, method='multistep'), 15),
                     singlestep3_15=(new(False, steps=15, order=3, method='singlestep'), 15))
        for name, (fn, nfe) in cases.items():
            def run(loop):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = fn(loop)
                torch.cuda.synchronize()
                return time.perf_counter() - t0, out
            outs = {loop: run(loop)[1] for loop in (False, True)}          # warm-up, and the bits
            times = {False: [], True: []}
            loops[0] = 0
            for _ in range(a.runs):
                for loop in (False, True):
                    times[loop].append(run(loop)[0])
            assert loops[0] == a.runs, 'the device loop did not take the sampling over'
            row = dict(case=name, evaluations=nfe, B=B, device_loop_samplings=loops[0], same_bits=bool(torch.equal(outs[False], outs[True])),
                       per_step_s=statistics.median(times[False]), device_loop_s=statistics.median(times[True]),
                       per_step_samples=times[False], device_loop_samples=times[True])
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
