"""Seeded inputs of the hybrid-conditioning tests (UNets fed cat([x] + c_concat, 1): DiffusionWrapper 'hybrid', ldm/models/diffusion/
ddpm.py:1838-1841), shared by tools/make_goldens.py (which feeds them to the reference's LatentDiffusion.apply_model) and by
tests/test_hybrid_host.py / tests/test_gpu_hybrid.py (oracle and HIP engine).  Regenerated from the seed, never stored."""
import numpy as np
import torch

import golden_inputs as gi
from fgdm_amd import synth

IN_CHANNELS = (9, 8)       # SD-v1 inpainting (latent | mask | masked-image latent), InstructPix2Pix (latent | image latent)
T = (981, 1)
PREFIX = 'model.diffusion_model.'


def cfg(in_channels, base=None):
    return dict(gi.SD_CFG if base is None else base, in_channels=in_channels)


def _normal(name, shape, seed=7):
    return torch.from_numpy(synth._rng(name, seed).standard_normal(shape, dtype=np.float32))


def x(B=2, H=8, W=8, seed=7):
    return _normal('hybrid.x', (B, 4, H, W), seed)


def ctx(B=2, seed=7):
    return _normal('hybrid.ctx', (B, 77, 768), seed)


def c_concat(Cc, B=2, H=8, W=8, seed=7):
    """Cc = 4: a plain N(0,1) image latent.  Otherwise an inpainting input: one binary mask channel (a rectangle per sample, 1 =
    repaint) followed by the masked-image latent, (1 - mask) * N(0,1), in the remaining Cc - 1 channels."""
    if Cc == 4:
        return _normal('hybrid.cc4', (B, 4, H, W), seed)
    mask = torch.zeros(B, 1, H, W)
    for b in range(B):
        mask[b, :, H // 4 + b % 2:3 * H // 4, W // 8 + b % 3:5 * W // 8 + b % 3] = 1.0
    return torch.cat([mask, (1.0 - mask) * _normal(f'hybrid.cc{Cc}', (B, Cc - 1, H, W), seed)], 1)


def params(shapes, prefix=PREFIX):
    """{prefix + key: tensor} from the synthetic generator, names hashed with the prefix as load_synth hashes them"""
    return {prefix + k: torch.from_numpy(synth.make_tensor(prefix + k, s)) for k, s in shapes.items()}
