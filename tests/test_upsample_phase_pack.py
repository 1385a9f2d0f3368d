"""The identity behind IG_CONV2_PHASE ("Upsample convs as four 2x2 phase GEMMs"), on the CPU: nearest-2x upsample + conv3x3 (zero padding 1) equals four 2x2
convolutions over the source image, one per output phase (a, b), whose taps are sums of the 3x3 taps.  `phase_kernels` is a numpy
transcription of csrc/engine_shared.h: up_phase_pack (the lib ABI does not expose packed weights: the packer's own bits are
covered by the op-level parity of tests/test_gpu_upsample_phase.py)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROWS = {0: ((0,), (1, 2)), 1: ((0, 1), (2,))}      # phase -> 3x3 taps summed into 2x2 tap 0 / 1


def phase_kernels(w):
    """w [N, C, 3, 3] -> [2, 2, N, C, 2, 2]: out[a, b, :, :, ty, tx] = sum of w[:, :, ky, kx] over ky in ROWS[a][ty], kx in ROWS[b][tx]"""
    out = np.zeros((2, 2) + w.shape[:2] + (2, 2), dtype=w.dtype)
    for a in (0, 1):
        for b in (0, 1):
            for ty in (0, 1):
                for tx in (0, 1):
                    for ky in ROWS[a][ty]:
                        for kx in ROWS[b][tx]:
                            out[a, b, :, :, ty, tx] += w[:, :, ky, kx]
    return out


def phase_conv(x, w):
    """x [B, C, H, W], w [N, C, 3, 3] (float64) -> [B, N, 2H, 2W]: tap (ty, tx) of phase (a, b) reads source pixel
    (i + a - 1 + ty, j + b - 1 + tx), zero outside the image; the result goes to output pixel (2i + a, 2j + b)"""
    B, C, H, W = x.shape
    pk = phase_kernels(w)
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    out = np.zeros((B, w.shape[0], 2 * H, 2 * W), dtype=x.dtype)
    for a in (0, 1):
        for b in (0, 1):
            acc = np.zeros((B, w.shape[0], H, W), dtype=x.dtype)
            for ty in (0, 1):
                for tx in (0, 1):
                    src = xp[:, :, a + ty:a + ty + H, b + tx:b + tx + W]      # padded index = source index + 1
                    acc += np.einsum('bchw,nc->bnhw', src, pk[a, b, :, :, ty, tx])
            out[:, :, a::2, b::2] = acc
    return out


@pytest.mark.parametrize('shape', [(2, 3, 5, 7, 4), (1, 2, 1, 1, 3), (1, 4, 2, 6, 2)], ids=['5x7', '1x1', '2x6'])
def test_phase_sum_reproduces_upsample_conv3(shape):
    B, C, H, W, N = shape
    rng = np.random.default_rng(7)
    x = rng.standard_normal((B, C, H, W))
    w = rng.standard_normal((N, C, 3, 3)).astype(np.float32).astype(np.float64)      # random fp32 kernels
    ref = F.conv2d(F.interpolate(torch.from_numpy(x), scale_factor=2, mode='nearest'), torch.from_numpy(w), padding=1).numpy()
    got = phase_conv(x, w)
    assert np.abs(got - ref).max() < 1e-12


def test_phase_taps_cover_every_3x3_tap_once():
    w = np.arange(9, dtype=np.float64).reshape(1, 1, 3, 3) + 1
    pk = phase_kernels(w)
    for a in (0, 1):
        for b in (0, 1):
            assert pk[a, b].sum() == w.sum()
