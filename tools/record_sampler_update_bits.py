"""Record tests/golden/sampler_update_bits.npz: fixed inputs and the outputs of the fused sampler updates and the loop step kernels
(the calls of tests/sampler_update_cases.py), bit for bit, from ONE build of the library.  Run it once, on a GPU, against a build of
the commit whose bits are to be kept, BEFORE the kernels change:

    FGDM_LIB=/path/to/libfgdm_hip_parent.so python tools/record_sampler_update_bits.py --commit <hash> [--out FILE]

FGDM_LIB selects the build (fgdm_amd/_lib.py; tools/ab_lib.sh shows the pattern); without it the build in the tree is recorded.
tests/test_gpu_sampler_update_bits.py replays the stored inputs against the build in the tree and asserts torch.equal."""
import argparse
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
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'sampler_update_bits.npz'))
    a = ap.parse_args()
    import sampler_update_cases as cases
    from fgdm_amd import _lib
    lib = _lib.load()
    arrays = {'commit': np.array(a.commit)}
    for n in cases.SIZES:
        host = cases.make_inputs(n)
        arrays.update({f'n{n}/in/{k}': v.numpy() for k, v in host.items()})
        arrays.update({f'n{n}/out/{k}': v.cpu().numpy() for k, v in cases.run(lib, host).items()})
    np.savez_compressed(a.out, **arrays)
    print(f'{a.out}: {len(arrays)} arrays from {os.environ.get("FGDM_LIB") or _lib.LIB_PATH} ({a.commit}), {os.path.getsize(a.out)} bytes')


if __name__ == '__main__':
    main()
