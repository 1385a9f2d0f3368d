"""Record tests/golden/ancestral_update_bits.npz: fixed inputs and the outputs of fgdm_ancestral_step (the calls of
tests/ancestral_update_cases.py), bit for bit, from ONE build of the library.  Run it once, on a GPU, against a build of the commit
whose bits are to be kept:

    FGDM_LIB=/path/to/libfgdm_hip_parent.so python tools/record_ancestral_update_bits.py --commit <hash> [--out FILE]

FGDM_LIB selects the build; without it the build in the tree is recorded.  The library is opened with ctypes alone and only
fgdm_ancestral_step is bound, so a build of a commit older than the binding in fgdm_amd/_lib.py can be recorded.
tests/test_gpu_ancestral_update_bits.py replays the stored inputs against the build in the tree and asserts torch.equal."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--commit', required=True, help='hash of the commit the selected build was made from (stored in the file)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'ancestral_update_bits.npz'))
    a = ap.parse_args()
    import torch  # noqa: F401  (its HIP runtime first, as in fgdm_amd/_lib.py)
    import ancestral_update_cases as cases
    path = os.path.abspath(os.environ.get('FGDM_LIB') or os.path.join(ROOT, 'fgdm_amd', 'libfgdm_hip.so'))
    fn = cases.bind(C.CDLL(path))
    arrays = {'commit': np.array(a.commit)}
    for n in cases.SIZES:
        host = cases.make_inputs(n)
        arrays.update({f'n{n}/in/{k}': v.numpy() for k, v in host.items()})
        arrays.update({f'n{n}/out/{k}': v.cpu().numpy() for k, v in cases.run(fn, host).items()})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **arrays)
    print(f'{a.out}: {len(arrays)} arrays from {path} ({a.commit}), {os.path.getsize(a.out)} bytes')


if __name__ == '__main__':
    main()
