"""The two-strand attention kernels against a RECORDING of their own output bits (tests/golden/two_strand_bits.json, made by
tools/record_two_strand_bits.py from a build of the commit named in the file, before the 16-wide and the 32-wide kernel became two
instantiations of one template): same seeded inputs, same calls (tests/two_strand_bits_cases.py), the sha256 of every output.  A
mismatch means that the order of the arithmetic moved; the recording is never made again to follow the kernel."""
import json
import os

import pytest

import two_strand_bits_cases as cases

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, 'golden', 'two_strand_bits.json')


@pytest.fixture(scope='module')
def recording():
    with open(GOLD) as f:
        return json.load(f)


def check(case, got, recording):
    cid = cases.case_id(case)
    want = recording['cases'][cid]
    assert got['kernel'] == cases.KERNEL_IDS[case[0]], f'{cid}: ran on kernel {got["kernel"]}'
    assert got['in'] == want['in'], f'{cid}: the generated inputs are not the recorded ones'
    assert got['out'] == want['out'], f'{cid}: output bits differ from those of {recording["commit"]}'


def test_the_recording_covers_the_cases(recording):
    assert len(cases.CASES) == 64 and sorted(recording['cases']) == sorted(cases.case_id(c) for c in cases.CASES)
    assert len(recording['commit']) >= 7


@pytest.mark.parametrize('case', [c for c in cases.CASES if c[3] == 'climb_9'], ids=cases.case_id)
def test_climbing_cases_take_the_rescale_branch(case):
    """every strand of a climbing case moves its offset, and so rescales O, on EVERY tile after the first (CPU emulation)"""
    assert bool(cases.rescaled_tiles(case).all())


@pytest.mark.gpu
@pytest.mark.parametrize('case', [c for c in cases.CASES if c[0] == 'w32'], ids=cases.case_id)
def test_32_wide_kernel_reproduces_the_recorded_bits(recording, case):
    from fgdm_amd import _lib
    check(case, cases.run(_lib.load(), case), recording)


@pytest.mark.gpu
def test_16_wide_kernel_reproduces_the_recorded_bits(recording):
    """FGDM_ATTN_DQ=1 is read once per process: a fresh interpreter runs the sixteen d = 40 cases and prints their hashes"""
    got = cases.run_16_wide()
    mine = [c for c in cases.CASES if c[0] == 'w16']
    assert len(mine) == 16 and sorted(got) == sorted(cases.case_id(c) for c in mine)
    for c in mine:
        check(c, got[cases.case_id(c)], recording)

