"""Measure the parity bound of tests/test_gpu_attention_maps.py on the CPU: the normwise error of a plain fp32 torch evaluation of
mean_heads softmax(Q K^T) against the float64 one over the test's cases, and 4x the worst as the bound.  Writes
profiles/attention_maps_parity_errors.txt (the kernel's own errors are appended there by the GPU run of the test)."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..', 'tests'))
import attention_maps_cases as MC  # noqa: E402

if __name__ == '__main__':
    errs, worst, bound = MC.measure_bound()
    lines = ['# fp32 torch vs float64, normwise relative error of maps [B, T, Tk] (tools/attention_maps_bound.py, CPU)']
    lines += [f'{MC.case_id(c)}: {e:.3e}' for c, e in zip(MC.CASES, errs)]
    lines += [f'worst fp32-vs-float64 error: {worst:.3e}', f'bound = {MC.MARGIN:g} x worst: {bound:.3e}']
    out = os.path.join(HERE, '..', 'profiles', 'attention_maps_parity_errors.txt')
    with open(out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines[-2:]))
