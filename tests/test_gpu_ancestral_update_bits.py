"""fgdm_ancestral_step (k_ancestral) against a RECORDING of its own outputs (tests/golden/ancestral_update_bits.npz, made by
tools/record_ancestral_update_bits.py from a build of the commit named in the file, before the kernel's arithmetic moved into the
ancestral_rn helper that k_ancestral_loop_step shares): same stored inputs, same calls (tests/ancestral_update_cases.py), every
output bit for bit.  tests/test_gpu_sampler_update_bits.py does this for the other update kernels; its recording does not hold this
one.  The tests between the device ancestral loop and the per-step route say that the two agree; this one says that the per-step
kernel did not move."""
import os

import numpy as np
import pytest
import torch

import ancestral_update_cases as cases

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ancestral_update_bits.npz')


@pytest.fixture(scope='module')
def recording():
    with np.load(GOLD) as z:
        return {k: z[k] for k in z.files}


def test_the_recording_is_of_the_commit_before_the_helper(recording):
    assert str(recording['commit']).startswith('96f3e0f')


@pytest.mark.parametrize('n', cases.SIZES)
def test_ancestral_step_reproduces_the_recorded_bits(recording, n):
    from fgdm_amd import _lib
    host = {k: torch.from_numpy(recording[f'n{n}/in/{k}']) for k in cases.INPUTS}
    got = cases.run(cases.bind(_lib.load()), host)
    want = {k[len(f'n{n}/out/'):]: v for k, v in recording.items() if k.startswith(f'n{n}/out/')}
    assert sorted(got) == sorted(want) and len(want) == 18
    for k in sorted(want):
        w = torch.from_numpy(want[k]).cuda()
        assert torch.equal(got[k], w), (k, int((got[k] != w).sum()), 'elements differ')
    # the cases are not all alike: the noise term, and the std == 0 term with noise handed over, are really there
    assert not torch.equal(got['unit_t500_noise'], got['unit_t500_no_noise'])
    assert torch.equal(got['unit_t500_std0'].abs(), got['unit_t500_no_noise'].abs())
