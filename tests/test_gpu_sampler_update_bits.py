"""The fused sampler updates and the three loop step kernels against a RECORDING of their own outputs
(tests/golden/sampler_update_bits.npz, made by tools/record_sampler_update_bits.py from a build of the commit named in the file,
before the kernels were rewritten on shared rounding helpers): same stored inputs, same calls (tests/sampler_update_cases.py), every
output bit for bit.  The tests between the loop route and the per-step route say that the two agree; this one says that neither
moved."""
import os

import numpy as np
import pytest
import torch

import sampler_update_cases as cases

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'sampler_update_bits.npz')


@pytest.fixture(scope='module')
def recording():
    with np.load(GOLD) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize('n', cases.SIZES)
def test_sampler_updates_reproduce_the_recorded_bits(recording, n):
    from fgdm_amd import _lib
    host = {k: torch.from_numpy(recording[f'n{n}/in/{k}']) for k in cases.INPUTS}
    got = cases.run(_lib.load(), host)
    want = {k[len(f'n{n}/out/'):]: v for k, v in recording.items() if k.startswith(f'n{n}/out/')}
    assert sorted(got) == sorted(want) and len(want) >= 50
    for k in sorted(want):
        w = torch.from_numpy(want[k]).cuda()
        assert torch.equal(got[k], w), (k, int((got[k] != w).sum()), 'elements differ')
