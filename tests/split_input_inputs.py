"""Seeded inputs and settings of the patch-wise fixtures (tests/golden/split_input_*.npz), shared by tools/make_goldens.py
(which feeds them to the imported reference) and the tests (HIP engine)."""
import torch

from fgdm_amd import synth

# (h, w, ks, stride, uf, tie_braker) of split_input_tables.npz, in file order: weighting_<i>, normalization_<i>
TABLES = ((24, 40, (16, 16), (8, 8), 1, False),
          (24, 40, (16, 8), (8, 8), 1, False),
          (16, 24, (8, 8), (4, 4), 8, False),
          (24, 40, (16, 16), (8, 8), 1, True))

UNET_KS, UNET_STRIDE = (16, 16), (8, 8)
VAE_KS, VAE_STRIDE, VQF = (8, 8), (4, 4), 8
T = [801, 801]


def split_params(ks, stride, tie_braker=False):
    return dict(ks=tuple(ks), stride=tuple(stride), vqf=VQF, patch_distributed_vq=True, tie_braker=tie_braker,
                clip_min_weight=0.01, clip_max_weight=0.5, clip_min_tie_weight=0.01, clip_max_tie_weight=0.5)


def unet_x():
    return torch.from_numpy(synth.latents(2, 24, 32, seed=2100))


def unet_ctx():
    return torch.from_numpy(synth.context(2, seed=2101))


def vae_z(w=24):
    """latent as the sampler returns it (scaled by scale_factor), [1, 4, 16, w]"""
    return torch.from_numpy(synth.latents(1, 16, w, seed=2200 + w)) * 0.18215
