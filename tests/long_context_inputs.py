"""Seeded inputs of the long-context fixtures (tests/golden/long_context*.npz, clip_hack_tokens.json), shared by
tools/make_goldens.py (which feeds them to the imported reference) and the tests (oracle / HIP engine)."""
import numpy as np
import torch

from fgdm_amd import synth

T = [981, 21]
TOKENS = (154, 231)            # two and three 77-token parts (cat(c_crossattn, 1); hack_everything's three chunks)
RAW_LENGTHS = (0, 10, 75, 76, 150, 151, 225, 300)      # raw prompt lengths around the chunk borders 75 / 150 / 225


def ctx(tokens, n=2):
    return torch.from_numpy(synth.context(n, seed=1000 + tokens, tokens=tokens))


def x(hw, n=2):
    return torch.from_numpy(synth.latents(n, hw, hw, seed=1100 + hw))


def hint(res, n=2):
    return torch.from_numpy(synth.hint(n, res=res, seed=1200))


def raw_tokens(length):
    """a raw token list (no special tokens) of the given length, ids below BOS"""
    return [int(v) for v in synth._rng('hack.raw', 1300 + length).integers(0, 49406, size=length)]
