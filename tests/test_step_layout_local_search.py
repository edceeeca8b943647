"""step_layout::LsOut (csrc/step_layout.h), the local search's step buffer: tests/support/ls_layout_check.cpp, built with
the host C++ compiler alone (no HIP, no GPU), as tests/test_step_layout.py does for the other layouts."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'support', 'ls_layout_check.cpp')
INC = os.path.join(ROOT, 'simple_mip_solver_amd', 'csrc')


def test_local_search_layout_matches_the_engine(tmp_path):
    cxx = os.environ.get('CXX') or shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.fail('no host C++ compiler (c++, g++ or clang++) to build the layout check with')
    exe = str(tmp_path / 'ls_layout_check')
    subprocess.run([cxx, '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror', '-I', INC, SRC, '-o', exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert ' 0 failed' in run.stdout, run.stdout
