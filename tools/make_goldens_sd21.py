#!/usr/bin/env python3
"""Golden vectors for the SD-2.1-base style networks (a fixed head width of 64, nn.Linear proj_in / proj_out, a 1024-wide context),
from the REFERENCE's own modules on the CPU in fp32 -- and once more under the emulated torch.autocast("cuda") policy, exactly as
tools/make_goldens.py does for its `_ac` fixtures, so that tests/common.py::check_net judges the engine against the measured floor.

The reference keeps its SD-2 capable modules under controlnet/ (controlnet/ldm/modules/attention.py: SpatialTransformer(use_linear),
controlnet/ldm/modules/diffusionmodules/openaimodel.py: UNetModel(num_head_channels, use_linear_in_transformer),
controlnet/cldm/cldm.py: ControlNet, ControlledUnetModel).  Runs only where the reference checkout is mounted (FGDM_REFERENCE).
Arrays and a key / shape list are written, nothing else; weights and inputs are regenerated from the seed (tests/sd21_inputs.py).

Writes tests/golden/sd21_nets.npz, sd21_st.npz (+ *_ac.npz) and tests/golden/param_keys_sd21.json.
Usage:  python tools/make_goldens_sd21.py"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_goldens as mg  # noqa: E402  (stubs, load_synth, ref_cfg, save: one recipe for every fixture)

import torch  # noqa: E402

import sd21_inputs as si  # noqa: E402  (make_goldens put tests/ on the path)


def _no_checkpoint(m):
    for mod in m.modules():
        if hasattr(mod, 'checkpoint'):
            mod.checkpoint = False
    return m


def g_param_keys():
    from controlnet.cldm.cldm import ControlNet, ControlledUnetModel
    sd = lambda m: {k: list(v.shape) for k, v in m.state_dict().items()}
    with torch.device('meta'):
        out = {'unet': sd(ControlledUnetModel(**mg.ref_cfg(si.SD21_SMALL))),
               'controlnet': sd(ControlNet(**mg.ref_cfg(si.SD21_SMALL, hint_channels=3)))}
    with open(os.path.join(mg.GOLD, 'param_keys_sd21.json'), 'w') as f:
        json.dump(out, f)
    print('wrote param_keys_sd21.json', {k: len(v) for k, v in out.items()})


def g_nets():
    from controlnet.cldm.cldm import ControlNet, ControlledUnetModel
    arrs = {}
    with torch.no_grad():
        x, ctx, t = si.get('x'), si.get('ctx'), torch.tensor(si.T_PAIR, dtype=torch.long)
        cu = _no_checkpoint(ControlledUnetModel(**mg.ref_cfg(si.SD21_SMALL)).eval())
        mg.load_synth(cu, 'sd21.')
        cn = _no_checkpoint(ControlNet(**mg.ref_cfg(si.SD21_SMALL, hint_channels=3)).eval())
        mg.load_synth(cn, 'sd21_cn.')
        arrs['t'] = t
        arrs['eps'] = cu(x=x, timesteps=t, context=ctx, control=None)
        ctrl = cn(x=x, hint=si.hint(), timesteps=t, context=ctx)
        arrs['eps_ctrl'] = cu(x=x, timesteps=t, context=ctx, control=[c * s for c, s in zip(ctrl, si.CTRL_SCALES)],
                              only_mid_control=False)
    mg.save('sd21_nets', **arrs)


def g_st():
    from controlnet.ldm.modules.attention import SpatialTransformer
    with torch.no_grad():
        m = _no_checkpoint(SpatialTransformer(320, 5, 64, depth=1, context_dim=1024, use_linear=True).eval())
        mg.load_synth(m, 'sd21_st.')
        y = m(si.get('st_x'), context=si.get('ctx'))
    mg.save('sd21_st', y=y)


def main():
    if not os.path.isdir(mg.REF):
        sys.exit(f'reference checkout not found at {mg.REF}')
    mg.install_stubs()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    from oracle import autocast
    g_param_keys()
    for fn in (g_nets, g_st):
        fn()
        mg.AC_SUFFIX = '_ac'
        try:
            with autocast.emulate() as mode:
                fn()
            print('   ', mode.stats)
        finally:
            mg.AC_SUFFIX = ''


if __name__ == '__main__':
    main()
