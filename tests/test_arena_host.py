"""The workspace allocator and its owning handles (fgdm_amd/csrc/arena.h) on the host: tools/arena_check.cpp, a stand-alone program
over malloc'ed slabs, built with the address and undefined-behaviour sanitizers where the compiler has them, and run."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']


def test_arena_check_program(tmp_path):
    cxx = next((c for c in ('c++', 'g++', 'clang++') if shutil.which(c)), None)
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'arena_check')
    cmd = [cxx, '-std=c++17', '-g', os.path.join(ROOT, 'tools', 'arena_check.cpp'), '-o', exe]
    if subprocess.run(cmd + SANITIZE, capture_output=True).returncode != 0:      # no sanitizer runtime: the plain program still checks every case
        subprocess.run(cmd, check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert 'all cases passed' in run.stdout
