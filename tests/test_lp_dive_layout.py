"""mipx::LpdiveOut (csrc/lpdive_kernels.hip.h), what comes down with a step of the LP dive:
tests/support/lpdive_layout_check.cpp, as tests/test_step_layout_local_search.py does for step_layout::LsOut.  The
layout lives beside the dive's kernels, so the check is built with hipcc, the compiler the library is built with; it
issues no HIP call and needs no GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'support', 'lpdive_layout_check.cpp')
INC = os.path.join(ROOT, 'simple_mip_solver_amd', 'csrc')


def test_lp_dive_view_matches_the_offsets(tmp_path):
    hipcc = shutil.which(os.environ.get('HIPCC') or 'hipcc') or shutil.which('/opt/rocm/bin/hipcc')   # (csrc/Makefile's default)
    if hipcc is None:
        pytest.fail('no hipcc to build the layout check with')
    exe = str(tmp_path / 'lpdive_layout_check')
    subprocess.run([hipcc, '--offload-arch=gfx950', '-x', 'hip', '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror',
                    '-I', INC, SRC, '-o', exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert ' 0 failed' in run.stdout and 'lpdive_layout: 36 checks' in run.stdout, run.stdout   # (12 per cap: 1, 3, 257)
