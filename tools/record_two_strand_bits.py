"""Record tests/golden/two_strand_bits.json: the sha256 of the fp16 output (and of the seeded inputs) of every case of
tests/two_strand_bits_cases.py, from ONE build of the library.  Run it once, on a GPU, against a build of the commit whose bits are
to be kept, BEFORE the kernels change:

    FGDM_LIB=/path/to/libfgdm_hip_parent.so python tools/record_two_strand_bits.py --commit <hash> [--out FILE]

FGDM_LIB selects the build (fgdm_amd/_lib.py); without it the build in the tree is recorded.  The 16-wide cases run in a child
interpreter under FGDM_ATTN_DQ=1, which inherits FGDM_LIB.  tests/test_gpu_two_strand_bits.py replays the cases against the build in
the tree and compares the hashes."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--commit', required=True, help='hash of the commit the selected build was made from (stored in the file)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'two_strand_bits.json'))
    a = ap.parse_args()
    import two_strand_bits_cases as cases
    from fgdm_amd import _lib
    got = cases.run_width(_lib.load(), 'w32')
    got.update(cases.run_16_wide())
    for c in cases.CASES:
        r = got[cases.case_id(c)]
        assert r['kernel'] == cases.KERNEL_IDS[c[0]], (cases.case_id(c), r['kernel'])
        if c[3] == 'climb_9':
            assert cases.rescaled_tiles(c).all(), cases.case_id(c)
    rec = {'commit': a.commit, 'cases': {cid: {'in': r['in'], 'out': r['out']} for cid, r in sorted(got.items())}}
    with open(a.out, 'w') as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write('\n')
    print(f'{a.out}: {len(rec["cases"])} cases from {os.environ.get("FGDM_LIB") or _lib.LIB_PATH} ({a.commit}), '
          f'{len({r["out"] for r in rec["cases"].values()})} distinct outputs')


if __name__ == '__main__':
    main()
