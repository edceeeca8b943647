"""The cube search (include/mipx_cube.h), the parts that need no GPU: the header against the ctypes table and the
exported symbols, what BranchAndBound refuses at construction, the layout of the option's step buffer, and the NumPy
restatement of the algorithm (tests/support/cube_search_reference.py): its pick against scipy's milp on the same cube,
and its VALIDITY on random data."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from scipy.optimize import Bounds, LinearConstraint, milp

from simple_mip_solver_amd import BranchAndBound, PseudoCostBranchNode, _ffi
from tests.support import cube_search_reference as ref
from tests.support.abi_check import agrees, prototypes
from tests.support.example_models import model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ['mipx_cube_search_batch', 'mipx_tree_set_cube_search', 'mipx_tree_cube_search_stats']


def test_cube_search_header_and_signature_table_agree():
    protos = prototypes('mipx_cube.h')
    assert sorted(protos) == sorted(_ffi.CUBE_SYMBOLS) == sorted(NAMES)
    for name, (ret, params) in protos.items():
        restype, argtypes = _ffi._CUBE_SIGNATURES[name]
        assert agrees(ret, restype), name
        assert len(params) == len(argtypes), name
        for k, (decl, ctype) in enumerate(zip(params, argtypes)):
            assert agrees(decl, ctype), f'{name} parameter {k} is `{decl}`, the table says {ctype}'


def test_new_symbols_overlap_no_existing_list():
    old = set(_ffi.SYMBOLS) | set(_ffi.SPILL_SYMBOLS) | set(_ffi.CUTMIG_SYMBOLS) | set(_ffi.DUALFN_SYMBOLS) | \
        set(_ffi.TREEREC_SYMBOLS) | set(_ffi.CGLP_SYMBOLS) | set(_ffi.RESTART_SYMBOLS) | set(_ffi.HEUR_SYMBOLS) | \
        set(_ffi.PROP_SYMBOLS) | set(_ffi.RCFIX_SYMBOLS) | set(_ffi.OBJSTEP_SYMBOLS) | set(_ffi.LSEARCH_SYMBOLS) | \
        set(_ffi.FIXPROP_SYMBOLS) | set(_ffi.WREPAIR_SYMBOLS)
    assert not set(_ffi.CUBE_SYMBOLS) & old


def test_mipx_h_includes_the_header_and_keeps_its_version():
    text = open(os.path.join(ROOT, 'include', 'mipx.h')).read()
    assert '#include "mipx_cube.h"' in text
    assert _ffi.lib().mipx_abi_version() == 1


def test_library_exports_the_entries():
    L = _ffi.lib()
    for name in _ffi.CUBE_SYMBOLS:
        assert hasattr(L, name), name
        assert getattr(L, name).restype is _ffi._CUBE_SIGNATURES[name][0]


def test_stats_keys_and_status_codes_cover_the_header():
    text = open(os.path.join(ROOT, 'include', 'mipx_cube.h')).read()
    assert [int(k) for k in re.findall(r'\[(\d)\] ', text)] == list(range(8))
    assert _ffi.CUBE_STATS_KEYS == ('points', 'found', 'none', 'columns', 'at_cap', 'incumbents', 'reserved6', 'kernel_us')
    codes = {name.lower(): int(v) for name, v in re.findall(r'#define MIPX_CUBE_(FOUND|NONE|SKIPPED) (\d)', text)}
    assert codes == {v: k for k, v in _ffi.CUBE_STATUS.items()} and len(codes) == 3
    assert (ref.FOUND, ref.NONE, ref.SKIPPED) == tuple(codes[k] for k in ('found', 'none', 'skipped'))
    # FOUND and SKIPPED are the heuristic's feasible and skipped: the engine gates the lift by the cube's status
    assert _ffi.HEUR_STATUS[codes['found']] == 'feasible' and _ffi.HEUR_STATUS[codes['skipped']] == 'skipped'
    assert int(re.search(r'#define MIPX_CUBE_MAX_COLUMNS (\d+)', text).group(1)) == _ffi.MAX_CUBE_SEARCH_COLUMNS == 20
    assert _ffi.DEFAULT_CUBE_SEARCH_COLUMNS == ref.MAX_COLUMNS == 16


def test_c_entries_refuse_null_arguments():
    L = _ffi.lib()
    assert L.mipx_cube_search_batch(None, 0, *([None] * 4), 0, np.inf, 1e-9, 1e-4, 16, *([None] * 5)) == -1   # MIPX_EINVAL
    assert L.mipx_tree_set_cube_search(None, 4) == -1
    assert L.mipx_tree_cube_search_stats(None, None) == -1


def test_step_buffer_layout_matches_the_engine(tmp_path):
    cxx = os.environ.get('CXX') or shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.fail('no host C++ compiler (c++, g++ or clang++) to build the layout check with')
    exe = str(tmp_path / 'cube_layout_check')
    subprocess.run([cxx, '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror', '-I', os.path.join(ROOT, 'simple_mip_solver_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'support', 'cube_layout_check.cpp'), '-o', exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert ' 0 failed' in run.stdout, run.stdout


# ---- what the constructor refuses ------------------------------------------------------------------------------
def build(**extra):
    kw = dict(pseudo_costs={}, frontier_batch=4, gomory_cuts=False, primal_heuristic=True, cube_search=True)
    kw.update(extra)
    return BranchAndBound(model('small_branch'), PseudoCostBranchNode, **kw)


@pytest.mark.parametrize('value', [False, 0, -3, 21, 2.5, 'on'])
def test_cube_search_value(value):
    with pytest.raises(ValueError, match='cube_search is None, True or a number of columns from 1 to 20'):
        build(cube_search=value)


def test_cube_search_needs_the_heuristic():
    with pytest.raises(ValueError, match='cube_search needs primal_heuristic'):
        build(primal_heuristic=None)
    with pytest.raises(AssertionError, match='primal_heuristic needs frontier_batch'):
        build(frontier_batch=None)
    with pytest.raises(AssertionError, match='primal_heuristic needs gomory_cuts=False'):
        build(gomory_cuts=True)
    with pytest.raises(AssertionError, match='primal_heuristic cannot be combined with comm'):
        build(comm=object())


def test_option_is_off_by_default_and_inherited_by_restart():
    on = build()
    assert on._cube_search is True and on.cube_search_stats is None and on._given['cube_search'] is True
    assert build(cube_search=7)._given['cube_search'] == 7 and build(cube_search=20)._cube_search == 20
    plain = build(cube_search=None)
    assert plain._cube_search is None and plain._given['cube_search'] is None and plain.cube_search_stats is None
    assert BranchAndBound(model('small_branch'), PseudoCostBranchNode, pseudo_costs={})._cube_search is None
    assert 'cube_search' in BranchAndBound._restart_overrides and 'primal_heuristic' in BranchAndBound._restart_overrides
    # (what it works beside)
    assert build(propagate=True, reduced_cost=True, objective_step=True, local_search=True, host_spill=1 << 24, dive=8,
                 anchor=False)._cube_search is True
    assert build(tree_record=True)._cube_search is True and build(dual_function=True)._cube_search is True
    assert build(fix_propagate=True)._cube_search is True and build(weighted_repair=True)._cube_search is True


def test_restart_without_the_heuristic_drops_the_option(monkeypatch):
    from simple_mip_solver_amd.lp import CyLPArray
    src = build(tree_record=True, local_search=True)
    src.status = 'optimal'
    seeded = []
    monkeypatch.setattr(BranchAndBound, '_seed_native', lambda self, source: seeded.append(self))
    b = CyLPArray(np.asarray(src.root_node.lp.constraints[0].lower, dtype=np.float64).copy())
    new = src.restart(b, primal_heuristic=None)
    assert new._primal_heuristic is None and new._cube_search is None and new._local_search is None and seeded == [new]
    kept = src.restart(b)
    assert kept._primal_heuristic is True and kept._cube_search is True and kept._local_search is True
    fewer = src.restart(b, cube_search=3)
    assert fewer._cube_search == 3 and fewer._primal_heuristic is True
    off = src.restart(b, cube_search=None)
    assert off._cube_search is None and off._local_search is True
    with pytest.raises(ValueError, match='cube_search needs primal_heuristic'):
        src.restart(b, primal_heuristic=None, cube_search=True)


# ---- the restatement -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', range(4))
def test_the_pick_has_the_objective_milp_finds_on_the_same_cube(seed):
    """40 x 20, the root LP point, K = 16: the columns outside F fixed at x~, those in F in [floor, floor + 1]; the
    data is integer, so the two objectives are the same number up to HiGHS's own arithmetic."""
    (A, b, c, l, u, ints), x0 = ref.root_point(40, 20, seed)
    d = {}
    xo, obj, status, (k, code) = ref.cube_search_one(A, b, c, l, u, ints, x0, detail=d)
    lo, hi = d['base'].copy(), d['base'].copy()
    hi[d['F']] += 1.0
    h = milp(c, constraints=LinearConstraint(A, lb=b, ub=np.inf), bounds=Bounds(lo, hi), integrality=np.ones(len(c)),
             options={'mip_rel_gap': 0.0})
    print(seed, 'k', k, 'code', code, 'status', status, 'obj', obj, 'milp', h.status, h.fun)
    assert k in (9, 10) and status == ref.FOUND and h.status == 0
    assert abs(obj - float(h.fun)) <= 1e-9 * max(1.0, abs(obj))
    ref.certify(A, b, c, l, u, ints, x0, xo, obj)
    # a cutoff at the pick's own objective leaves only worse codes out and this one too: NONE below it, the pick above
    assert ref.cube_search_one(A, b, c, l, u, ints, x0, cutoff=obj)[2] == ref.NONE
    again = ref.cube_search_one(A, b, c, l, u, ints, x0, cutoff=obj + 0.5)
    assert again[2] == ref.FOUND and again[3] == (k, code)


def random_case(seed, m=7, n=12, n_int=9):
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(m, n)).round(3)
    c = rng.normal(size=n).round(3)
    l = np.zeros(n)
    u = np.full(n, 4.0)
    ints = np.sort(rng.choice(n, n_int, replace=False))
    xs = rng.uniform(0.0, 4.0, n)
    xr = xs.copy()
    xr[ints] = np.round(xs[ints])
    b = A @ xr - rng.uniform(0.0, 1.5, m)   # (the point with its integer columns rounded satisfies every row)
    return A, b, c, l, u, ints, xs


def brute_force(A, b, c, F, base, cutoff, tol):
    """The smallest (obj, code) over the cube by np.dot on every point: arithmetic of its own."""
    best = None
    for e in range(1 << len(F)):
        xo = base.copy()
        for t, j in enumerate(F):
            xo[j] += (e >> t) & 1
        if np.all(A @ xo - b >= -tol) and c @ xo < cutoff and (best is None or c @ xo < best[0] - 1e-9):
            best = (float(c @ xo), e)
    return best


@pytest.mark.parametrize('seed', range(12))
def test_validity_on_random_data_with_non_integer_matrix(seed):
    A, b, c, l, u, ints, x = random_case(seed)
    K = (3, 6, 16)[seed % 3]
    d = {}
    xo, obj, status, (k, code) = ref.cube_search_one(A, b, c, l, u, ints, x, max_columns=K, ftol=1e-4, detail=d)
    F = d['F']
    f = np.abs(x[ints] - np.floor(x[ints] + 0.5))
    assert k == len(F) == min(K, int((f > 1e-4).sum())) and list(F) == sorted(F)
    # F holds the k most fractional columns: none outside it is more fractional than one inside
    inside = np.isin(ints, F)
    assert k == 0 or inside.all() or f[inside].min() >= f[~inside].max()
    want = brute_force(A, b, c, F, d['base'], np.inf, 1e-9)
    if want is None:
        assert status == ref.NONE and code == -1 and obj == 0.0 and np.array_equal(xo.view(np.int64), x.view(np.int64))
    else:
        assert status == ref.FOUND and abs(obj - want[0]) <= 1e-9
        ref.certify(A, b, c, l, u, ints, x, xo, obj)
        assert np.array_equal(xo[F] - d['base'][F], [(code >> t) & 1 for t in range(k)])


def test_restatement_edges():
    A = np.array([[1.0, 1.0], [-1.0, -1.0], [1.0, 0.0]]); b = np.array([1.0, -3.0, 0.0]); c = np.array([1.0, 2.0])
    l = np.zeros(2); u = np.full(2, 5.0)
    # k = 0: every column integral; the cube is the rounded point alone
    assert ref.cube_search_one(A, b, c, l, u, [0, 1], [1.0, 1.0])[1:] == (3.0, ref.FOUND, (0, 0))
    assert ref.cube_search_one(A, b, c, l, u, [0, 1], [0.0, 0.0])[1:] == (0.0, ref.NONE, (0, -1))
    # k = 1: x0 = 0.5 goes down (row 0 broken with x1 = 0) or up
    xo, obj, status, counts = ref.cube_search_one(A, b, c, l, u, [0, 1], [0.5, 0.0])
    assert list(xo) == [1.0, 0.0] and (obj, status, counts) == (1.0, ref.FOUND, (1, 1))
    # a candidate refused by its bounds: u0 = 0.5 rounds to 0, so floor + 1 is outside and the column takes its ROUND
    xo, obj, status, counts = ref.cube_search_one(A, b, c, l, [0.5, 5.0], [0, 1], [0.5, 0.5])
    assert list(xo) == [0.0, 1.0] and (obj, status, counts) == (2.0, ref.FOUND, (1, 1))
    # u = +inf is a bound like any other
    assert ref.cube_search_one(A, b, c, l, [np.inf, np.inf], [0, 1], [0.5, 0.5])[3][0] == 2
    # the cap and its tie rule: three columns at f = 0.5, K = 2 keeps the two lower ones
    d = {}
    ref.cube_search_one(np.zeros((0, 3)), [], [1.0, 1.0, 1.0], np.zeros(3), np.full(3, 5.0), [0, 1, 2], [0.5, 1.5, 2.5], max_columns=2, detail=d)
    assert list(d['F']) == [0, 1] and list(d['base']) == [0.0, 1.0, 3.0]
    # all c equal: the objective ties and the lower code wins
    A1 = np.array([[1.0, 1.0]]); b1 = np.array([1.0])
    assert ref.cube_search_one(A1, b1, [1.0, 1.0], np.zeros(2), np.full(2, 5.0), [0, 1], [0.5, 0.5])[3] == (2, 1)
    # the batch: a skip mask
    o = ref.cube_search(A1, b1, [1.0, 1.0], np.zeros(2), np.full(2, 5.0), [0, 1], [[0.5, 0.5]] * 2, skip=[1, 0])
    assert list(o['status']) == [ref.SKIPPED, ref.FOUND] and o['counts'].tolist() == [[0, -1], [2, 1]]
    assert list(o['x'][0]) == [0.5, 0.5] and list(o['obj']) == [0.0, 1.0]
