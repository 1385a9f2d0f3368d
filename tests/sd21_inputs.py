"""Configs and seeded inputs of the SD-2.1-base style fixtures (tests/golden/sd21_*.npz, param_keys_sd21.json), shared by
tools/make_goldens_sd21.py (which feeds them to the imported reference) and by the tests.  Nothing but the reference's outputs is
stored: inputs and weights are regenerated from the seed, as for the fixtures of golden_inputs.py."""
import numpy as np
import torch

import golden_inputs as gi
from fgdm_amd import synth

# SMALL_CFG with the three SD-2.x differences: a fixed head WIDTH (320 / 640 channels: 5 and 10 heads, so the head count differs by
# level), nn.Linear proj_in / proj_out, and the 1024-wide context of the OpenCLIP text tower
SD21_SMALL = dict(gi.SMALL_CFG, num_heads=-1, num_head_channels=64, use_linear_in_transformer=True, context_dim=1024)
T_PAIR = (981, 21)              # one high, one low timestep
HINT_SEED = 48
CTRL_SCALES = gi.CTRL_SCALES    # 13 control scales, not all 1

# key -> (rng stream name, shape)
TABLE = {
    'x': ('sd21.x', (2, 4, 16, 16)),
    'ctx': ('sd21.ctx', (2, 77, 1024)),
    'st_x': ('sd21.st.x', (2, 320, 16, 16)),
}


def get(key, seed=7):
    name, shape = TABLE[key]
    return torch.from_numpy(synth._rng(name, seed).standard_normal(shape, dtype=np.float32))


def hint():
    return gi.hint(2, 128, HINT_SEED)        # 8 x the 16 x 16 latent


def rename(k):
    """engine state-dict key -> the name the generator hashed the synthetic weights with"""
    return k.replace('model.diffusion_model.', 'sd21.').replace('control_model.', 'sd21_cn.')
