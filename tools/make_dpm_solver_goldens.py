#!/usr/bin/env python3
"""Record tests/golden/dpm_solver.npz: the final x of the REFERENCE's own DPM_Solver.sample
(ldm/models/diffusion/dpm_solver/dpm_solver.py) with the analytic model of tools/make_goldens.py, for every configuration of
tests/dpm_solver_cases.py, and the number of model calls of each.  Like tools/make_goldens.py it runs only where the reference
checkout is mounted (FGDM_REFERENCE); only data is written.

Two lines of that module cannot run as they stand, and both are worked round HERE, in the generator, never in the product:
  * get_orders_and_timesteps_for_singlestep_solver calls torch.cumsum without `dim` (a TypeError with any torch); the generator
    supplies dim=0, the only reading of a cumulative sum over a 1-d tensor;
  * multistep order 3 with lower_order_final and steps < 15 hands three model values to the second-order update, which unpacks two
    (a ValueError).  Those cases are recorded as '<case>_raises' and have no trajectory.

Usage:  python tools/make_dpm_solver_goldens.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens as mg  # noqa: E402  (puts the repository and tests/ on sys.path)

import dpm_solver_cases as cases  # noqa: E402


def main():
    if not os.path.isdir(mg.REF):
        sys.exit(f'reference checkout not found at {mg.REF}')
    mg.install_stubs()
    from ldm.models.diffusion.dpm_solver.dpm_solver import NoiseScheduleVP, model_wrapper, DPM_Solver
    from fgdm_amd import schedule
    cumsum = torch.cumsum
    torch.cumsum = lambda t, dim=0, **kw: cumsum(t, dim, **kw)
    gi = mg.gi
    x_T, c, uc = gi.get('samp/x_T'), gi.get('samp/c'), gi.get('samp/uc')
    ns = NoiseScheduleVP('discrete', alphas_cumprod=torch.as_tensor(schedule.ddpm_tables()['alphas_cumprod'], dtype=torch.float32))
    arrs = {}
    for name, (px0, scale, kw) in cases.CASES.items():
        calls = [0]

        def model(x, t, cond):
            calls[0] += 1
            return mg.analytic_eps(x, t, cond)
        fn = model_wrapper(model, ns, model_type='noise', guidance_type='classifier-free', condition=c, unconditional_condition=uc,
                           guidance_scale=scale)
        try:
            with torch.no_grad():
                out = DPM_Solver(fn, ns, predict_x0=px0).sample(x_T, **kw)
        except ValueError as err:
            arrs[name + '_raises'] = np.asarray([type(err).__name__])
            print(f'{name}: the reference raises {type(err).__name__}: {err}')
            continue
        arrs[name] = out
        arrs[name + '_calls'] = np.asarray([calls[0]])
    torch.cumsum = cumsum
    mg.save('dpm_solver', **arrs)


if __name__ == '__main__':
    main()
