"""A refused evaluation gives its workspace back: every block of the activation arenas is held by an owning handle
(fgdm_amd/csrc/arena.h), so a call that returns an error code in the middle of a forward pass unwinds what it holds.

The reduced synthetic engine (golden_inputs.SMALL_CFG) with one ControlNet; the FG-DM adapter exists for the SD-v1 topology only
(model.h refuses it on any other), so the refusal used here is the ControlNet's: a hint cached for a 16 x 16 latent and an
evaluation at 8 x 8.  controlnet_fwd checks that on the host, in front of its first launch, when the evaluation already holds its
input, context and embedding blocks -- and, with FGDM_PAIR_LAUNCH=0, every skip tensor of the UNet encoder, and, with
FGDM_TWIN_STREAMS=1, on the second stream behind the fork.  Every launch before the refusal has a valid geometry; the refused call
is the smaller one, so it cannot raise the peak by itself."""
import os
import subprocess
import sys

import pytest
import torch

import golden_inputs as gi
from fgdm_amd import synth

pytestmark = pytest.mark.gpu


def _run(refuse):
    """outputs of the good calls and the workspace figures after (good, [refused,] good) on a fresh engine"""
    from fgdm_amd.engine import Engine
    B = 2
    x, ctx = torch.from_numpy(synth.latents(B, 16, 16, seed=71)), torch.from_numpy(synth.context(B, seed=72))
    hint, t = torch.from_numpy(synth.hint(B, res=128, seed=73)), torch.tensor([981, 21])
    e = Engine(gi.SMALL_CFG, n_controlnets=1)
    try:
        for k, shape in e.param_shapes().items():
            e.load_tensor(k, synth.make_tensor(k, shape))
        e.finalize()
        e.set_hint(0, hint)
        outs = [e.apply_model(x, t, ctx).cpu()]
        handed_out = e.workspace_stats()['peak_bytes']
        if refuse:
            with pytest.raises(RuntimeError, match=r'fgdm_apply_model failed \(-\d+\): cached hint does not match'):
                e.apply_model(x[:, :, :8, :8].contiguous(), t, ctx)
            torch.cuda.synchronize()
        outs.append(e.apply_model(x, t, ctx).cpu())
        return outs, handed_out, e.workspace_stats()
    finally:
        e.close()


def test_refused_evaluation_leaves_nothing_behind():
    (first, again), handed_out, stats = _run(refuse=True)
    (want, _), _, clean = _run(refuse=False)
    print(f'workspace after good, refused, good: {stats}; after good, good: {clean}')
    assert handed_out > 0
    assert torch.isfinite(first).all() and torch.equal(first, want)
    assert torch.equal(again, first)
    assert stats['peak_bytes'] == clean['peak_bytes'] and stats['reserved_bytes'] == clean['reserved_bytes'], (stats, clean)


@pytest.mark.parametrize('knob,value', [('FGDM_TWIN_STREAMS', '1'), ('FGDM_PAIR_LAUNCH', '0')])
def test_refused_evaluation_under_the_other_schedules(knob, value):
    """The same on the second stream (the refusal comes behind the fork: the guard in apply_model_walk drains that stream before a
    block goes back) and with the ControlNet behind the whole UNet encoder.  The knobs are read once: a fresh interpreter."""
    env = dict(os.environ, **{knob: value})
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-q', '-x', '-m', 'gpu', '-k', 'leaves_nothing_behind'],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
