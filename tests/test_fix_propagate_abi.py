"""The fix-and-propagate dive (include/mipx_fixprop.h), the parts that need no GPU: the header against the ctypes table
and the exported symbols, what BranchAndBound refuses at construction, the layout of the dive's step buffer, and the
NumPy restatement of the algorithm (tests/support/fix_propagate_reference.py) against brute force and against the
rounding heuristic on the instances where that one is stuck."""
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from simple_mip_solver_amd import BranchAndBound, PseudoCostBranchNode, _ffi
from simple_mip_solver_amd.generators import random_dense_milp_arrays
from tests.support import fix_propagate_reference as ref
from tests.support import heuristic_reference as heur
from tests.support.abi_check import agrees, prototypes
from tests.support.example_models import model
from tests.support.propagation_reference import mixed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ['mipx_fix_propagate_batch', 'mipx_tree_set_fix_propagate', 'mipx_tree_fix_propagate_stats']


def test_fix_propagate_header_and_signature_table_agree():
    protos = prototypes('mipx_fixprop.h')
    assert sorted(protos) == sorted(_ffi.FIXPROP_SYMBOLS) == sorted(NAMES)
    for name, (ret, params) in protos.items():
        restype, argtypes = _ffi._FIXPROP_SIGNATURES[name]
        assert agrees(ret, restype), name
        assert len(params) == len(argtypes), name
        for k, (decl, ctype) in enumerate(zip(params, argtypes)):
            assert agrees(decl, ctype), f'{name} parameter {k} is `{decl}`, the table says {ctype}'


def test_new_symbols_overlap_no_existing_list():
    old = set(_ffi.SYMBOLS) | set(_ffi.SPILL_SYMBOLS) | set(_ffi.CUTMIG_SYMBOLS) | set(_ffi.DUALFN_SYMBOLS) | \
        set(_ffi.TREEREC_SYMBOLS) | set(_ffi.CGLP_SYMBOLS) | set(_ffi.RESTART_SYMBOLS) | set(_ffi.HEUR_SYMBOLS) | \
        set(_ffi.PROP_SYMBOLS) | set(_ffi.RCFIX_SYMBOLS) | set(_ffi.OBJSTEP_SYMBOLS) | set(_ffi.LSEARCH_SYMBOLS)
    assert not set(_ffi.FIXPROP_SYMBOLS) & old


def test_mipx_h_includes_the_header_and_keeps_its_version():
    text = open(os.path.join(ROOT, 'include', 'mipx.h')).read()
    assert '#include "mipx_fixprop.h"' in text
    assert _ffi.lib().mipx_abi_version() == 1


def test_library_exports_the_entries():
    L = _ffi.lib()
    for name in _ffi.FIXPROP_SYMBOLS:
        assert hasattr(L, name), name
        assert getattr(L, name).restype is _ffi._FIXPROP_SIGNATURES[name][0]


def test_stats_keys_and_status_codes_cover_the_header():
    text = open(os.path.join(ROOT, 'include', 'mipx_fixprop.h')).read()
    assert [int(k) for k in re.findall(r'\[(\d)\] ', text)] == list(range(8))
    assert _ffi.FIXPROP_STATS_KEYS == ('points', 'feasible', 'stuck', 'capped', 'fixings', 'tries', 'incumbents', 'kernel_us')
    codes = {name.lower(): int(v) for name, v in re.findall(r'#define MIPX_FP_(\w+) (\d)', text)}
    assert codes == {v: k for k, v in _ffi.FIXPROP_STATUS.items()} and len(codes) == 6
    assert (ref.FEASIBLE, ref.STUCK, ref.CAPPED, ref.SKIPPED, ref.INFEASIBLE_BOX, ref.ROWS) == \
        tuple(codes[k] for k in ('feasible', 'stuck', 'capped', 'skipped', 'infeasible_box', 'rows'))
    # the first four are the heuristic's codes: the engine gates either kernel by the other's status
    assert [codes[k] for k in ('feasible', 'stuck', 'capped', 'skipped')] == [k for k, _ in sorted(_ffi.HEUR_STATUS.items())]
    assert _ffi.DEFAULT_FIX_PROPAGATE_TRIES == ref.MAX_TRIES == 256 and _ffi.DEFAULT_FIX_PROPAGATE_ROUNDS == ref.MAX_ROUNDS == 8


def test_c_entries_refuse_null_arguments():
    L = _ffi.lib()
    assert L.mipx_fix_propagate_batch(None, 0, *([None] * 4), 0, np.inf, 1e-9, 8, 4, *([None] * 5)) == -1   # MIPX_EINVAL
    assert L.mipx_tree_set_fix_propagate(None, 8, 4) == -1
    assert L.mipx_tree_fix_propagate_stats(None, None) == -1


def test_step_buffer_layout_matches_the_engine(tmp_path):
    cxx = os.environ.get('CXX') or shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.fail('no host C++ compiler (c++, g++ or clang++) to build the layout check with')
    exe = str(tmp_path / 'fp_layout_check')
    subprocess.run([cxx, '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror', '-I', os.path.join(ROOT, 'simple_mip_solver_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'support', 'fp_layout_check.cpp'), '-o', exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert ' 0 failed' in run.stdout, run.stdout


# ---- what the constructor refuses ------------------------------------------------------------------------------
def build(**extra):
    kw = dict(pseudo_costs={}, frontier_batch=4, gomory_cuts=False, primal_heuristic=True, fix_propagate=True)
    kw.update(extra)
    return BranchAndBound(model('small_branch'), PseudoCostBranchNode, **kw)


@pytest.mark.parametrize('value', [False, 0, -3, 2.5, 'on'])
def test_fix_propagate_value(value):
    with pytest.raises(AssertionError, match='fix_propagate is None, True or a positive number of tries'):
        build(fix_propagate=value)


def test_fix_propagate_needs_the_heuristic():
    with pytest.raises(AssertionError, match='fix_propagate needs primal_heuristic'):
        build(primal_heuristic=None)
    with pytest.raises(AssertionError, match='primal_heuristic needs frontier_batch'):   # (and so frontier_batch and no cut rounds)
        build(frontier_batch=None)
    with pytest.raises(AssertionError, match='primal_heuristic needs gomory_cuts=False'):
        build(gomory_cuts=True)
    with pytest.raises(AssertionError, match='primal_heuristic cannot be combined with comm'):
        build(comm=object())


def test_option_is_off_by_default_and_inherited_by_restart():
    on = build()
    assert on._fix_propagate is True and on.fix_propagate_stats is None and on._given['fix_propagate'] is True
    assert build(fix_propagate=7)._given['fix_propagate'] == 7
    plain = build(fix_propagate=None)
    assert plain._fix_propagate is None and plain._given['fix_propagate'] is None and plain.fix_propagate_stats is None
    assert BranchAndBound(model('small_branch'), PseudoCostBranchNode, pseudo_costs={})._fix_propagate is None
    assert 'fix_propagate' in BranchAndBound._restart_overrides and 'primal_heuristic' in BranchAndBound._restart_overrides
    # (what it works beside)
    assert build(propagate=True, reduced_cost=True, objective_step=True, local_search=True, host_spill=1 << 24, dive=8,
                 anchor=False)._fix_propagate is True
    assert build(tree_record=True)._fix_propagate is True and build(dual_function=True)._fix_propagate is True


def test_restart_without_the_heuristic_drops_the_dive(monkeypatch):
    from simple_mip_solver_amd.lp import CyLPArray
    src = build(tree_record=True, local_search=True)
    src.status = 'optimal'
    seeded = []
    monkeypatch.setattr(BranchAndBound, '_seed_native', lambda self, source: seeded.append(self))
    b = CyLPArray(np.asarray(src.root_node.lp.constraints[0].lower, dtype=np.float64).copy())
    new = src.restart(b, primal_heuristic=None)
    assert new._primal_heuristic is None and new._fix_propagate is None and new._local_search is None and seeded == [new]
    kept = src.restart(b)
    assert kept._primal_heuristic is True and kept._fix_propagate is True and kept._local_search is True
    fewer = src.restart(b, fix_propagate=3)
    assert fewer._fix_propagate == 3 and fewer._primal_heuristic is True
    off = src.restart(b, fix_propagate=None)
    assert off._fix_propagate is None and off._local_search is True
    with pytest.raises(AssertionError, match='fix_propagate needs primal_heuristic'):
        src.restart(b, primal_heuristic=None, fix_propagate=True)


# ---- the restatement against brute force -------------------------------------------------------------------------
def integer_points(l, u):
    return (np.array(p, dtype=np.float64) for p in itertools.product(*[range(int(lo), int(up) + 1) for lo, up in zip(l, u)]))


def small_problem(rng):
    """3 to 5 integer columns in boxes inside 0..3, rows that pack and rows that cover, integer data."""
    n, m = int(rng.integers(3, 6)), int(rng.integers(1, 5))
    A = rng.integers(0, 5, (m, n)).astype(np.float64) * np.where(rng.random(m) < 0.5, 1.0, -1.0)[:, None]
    c = rng.integers(-6, 7, n).astype(np.float64)
    l = rng.integers(0, 2, n).astype(np.float64)
    u = np.minimum(3.0, l + rng.integers(0, 4, n))
    inside = np.floor(l + rng.random(n) * (u - l + 1))
    b = A @ inside - rng.integers(-2, 4, m)   # (now and then no point of the box satisfies the rows)
    x = l + rng.random(n) * (u - l)
    return A, b, c, l, u, list(range(n)), x


def test_restatement_by_brute_force_on_small_boxes():
    rng = np.random.default_rng(11)
    seen = np.zeros(6, np.int64)
    boxes_proven_empty = 0
    for trial in range(300):
        A, b, c, l, u, ints, x = small_problem(rng)
        objs = [float(c @ p) for p in integer_points(l, u) if np.all(A @ p - b >= -ref.TOL)]
        for cutoff in (np.inf, (float(np.median(objs)) if objs else 0.0), (min(objs) - 1.0 if objs else -100.0)):
            xt, obj, status, (fixings, tries), _ = ref.fix_propagate_one(A, b, c, l, u, ints, x, cutoff=cutoff)
            seen[status] += 1
            within = [o for o in objs if o <= cutoff + ref.TOL]
            assert status in (ref.FEASIBLE, ref.STUCK, ref.INFEASIBLE_BOX)   # (all columns integer, exact data: never ROWS)
            assert tries >= fixings and fixings <= len(ints)
            if status == ref.FEASIBLE:
                heur.certify(A, b, c, l, u, ints, xt, obj, tol=ref.TOL)
                assert obj <= cutoff + ref.TOL and within and obj >= min(within)
            else:
                assert np.array_equal(xt, x) and obj == 0.0
            if status == ref.INFEASIBLE_BOX:
                assert not within and (fixings, tries) == (0, 0)
                boxes_proven_empty += 1
    print(seen, boxes_proven_empty)
    assert seen[ref.FEASIBLE] > 300 and seen[ref.STUCK] >= 5 and boxes_proven_empty > 100   # (the outcomes are all exercised)


@pytest.mark.parametrize('family', ['generator', 'mixed'])
def test_restatement_by_brute_force_at_8_by_4(family):
    """8 x 4 with the bounds cut to 0..2 (3^8 points to enumerate), from LP-like points."""
    rng = np.random.default_rng(3)
    seen = np.zeros(6, np.int64)
    for seed in range(6):
        A, b, c, l, u, ints = ref.instance(family, 8, 4, seed)
        u = np.minimum(u, 2.0)
        b = np.ceil(b * 0.2)
        pts = np.array(list(integer_points(l, u)))
        ok = np.all(pts @ A.T - b >= -ref.TOL, axis=1)
        objs = pts[ok] @ c
        for k in range(12):
            x = l + rng.random(8) * (u - l)
            cutoff = np.inf if k % 3 == 0 or not objs.size else float(np.quantile(objs, 0.1 * (k % 4)))
            xt, obj, status, counts, _ = ref.fix_propagate_one(A, b, c, l, u, ints, x, cutoff=cutoff, max_tries=(3 if k == 11 else 256))
            seen[status] += 1
            within = objs[objs <= cutoff + ref.TOL]
            if status == ref.FEASIBLE:
                heur.certify(A, b, c, l, u, ints, xt, obj, tol=ref.TOL)
                assert obj <= cutoff + ref.TOL and obj >= within.min()
            if status == ref.INFEASIBLE_BOX:
                assert within.size == 0
            if status == ref.CAPPED:
                assert counts == (3, 3) or counts[1] == 3
    print(family, seen)
    assert seen[ref.FEASIBLE] > 20 and seen[ref.CAPPED] >= 1 and seen[ref.ROWS] == 0


def test_restatement_edges():
    # x0 + x1 >= 3 and x0 + x1 <= 3 in 0..5: from (0.2, 0.4) x0 -> 0, then x1 is fixed by the propagation alone
    A = np.array([[1.0, 1.0], [-1.0, -1.0]]); b = np.array([3.0, -3.0]); c = np.array([1.0, 2.0]); l = np.zeros(2); u = np.full(2, 5.0)
    xt, obj, status, counts, _ = ref.fix_propagate_one(A, b, c, l, u, [0, 1], [0.2, 0.4])
    assert list(xt) == [0.0, 3.0] and obj == 6.0 and status == ref.FEASIBLE and counts == (1, 1)
    # the values of a column in ascending distance, ties to the smaller: 2 x0 = 6 from 0.5 tries 0, 1, then -1 (outside), 2, 3
    A = np.array([[2.0], [-2.0]]); b = np.array([6.0, -6.0])
    xt, obj, status, counts, _ = ref.fix_propagate_one(A, b, [1.0], [0.0], [5.0], [0], [0.5])
    assert list(xt) == [3.0] and status == ref.FEASIBLE and counts == (0, 0)   # (START alone fixes it)
    # ... and with propagation too weak to see it (one round, two columns): the walk finds the value
    A = np.array([[1.0, 1.0], [-1.0, -1.0], [1.0, -1.0], [-1.0, 1.0]]); b = np.array([4.0, -4.0, 0.0, 0.0])
    out = ref.fix_propagate_one(A, b, [0.0, 0.0], [0.0, 0.0], [4.0, 4.0], [0, 1], [0.4, 0.0], max_rounds=1)
    assert list(out[0]) == [2.0, 2.0] and out[2] == ref.FEASIBLE and out[3][1] > out[3][0]   # (0 and 1 are refused first)
    assert ref.fix_propagate_one(A, b, [0.0, 0.0], [0.0, 0.0], [4.0, 4.0], [0, 1], [0.4, 0.0], max_rounds=1, max_tries=1)[2] == ref.CAPPED
    assert ref.fix_propagate_one(A, b, [0.0, 0.0], [0.0, 0.0], [4.0, 4.0], [0, 1], [0.4, 0.0], max_tries=0)[2] in (ref.CAPPED, ref.FEASIBLE)
    # an empty box, by the rows and by the cutoff
    assert ref.fix_propagate_one(np.array([[1.0]]), [7.0], [1.0], [0.0], [5.0], [0], [2.0])[2] == ref.INFEASIBLE_BOX
    assert ref.fix_propagate_one(np.array([[1.0]]), [2.0], [1.0], [0.0], [5.0], [0], [2.0], cutoff=1.5)[2] == ref.INFEASIBLE_BOX
    assert ref.fix_propagate_one(np.array([[1.0]]), [2.0], [1.0], [0.0], [5.0], [0], [2.0], cutoff=2.0)[:3] == (np.array([2.0]), 2.0, ref.FEASIBLE)
    # fractional bounds are rounded as the heuristic rounds them; no integer column at all: the clamped point, checked
    assert list(ref.fix_propagate_one(np.zeros((0, 1)), [], [1.0], [0.25], [3.75], [0], [0.0])[0]) == [1.0]
    out = ref.fix_propagate_one(np.array([[1.0]]), [2.0], [1.0], [0.0], [5.0], [], [1.5])
    assert list(out[0]) == [1.5] and out[2] == ref.ROWS and out[1] == 1.5
    # a continuous column whose clamped value breaks a row the integers cannot mend: ROWS, with the point
    out = ref.fix_propagate_one(np.array([[1.0, 1.0]]), [5.0], [1.0, 1.0], [0.0, 0.0], [2.0, 9.0], [0], [0.3, 1.0])
    assert out[2] == ref.ROWS and list(out[0]) == [0.0, 1.0] and out[1] == 1.0
    # the batch: a skipped point comes back unchanged with obj 0
    o = ref.fix_propagate(np.array([[1.0]]), [2.0], [1.0], [0.0], [5.0], [0], [[2.5], [2.5]], skip=[1, 0])
    assert list(o['status']) == [ref.SKIPPED, ref.FEASIBLE] and o['obj'][0] == 0.0 and o['x'][0, 0] == 2.5 and not o['counts'][0].any()


# ---- the dive where the rounding heuristic is stuck ----------------------------------------------------------------
# per seed of mixed(40, 20, 10, seed), on the root LP point and seven child LP points (ref.lp_points), with the
# engine's tolerance 1e-9: (points the rounding ends STUCK on, of those the dive ends FEASIBLE on), as the restatements
# give them
COMPLEMENT = {0: (7, 7), 1: (2, 2), 2: (8, 4), 3: (1, 1), 4: (5, 3), 5: (4, 4)}


@pytest.mark.parametrize('seed', range(6))
def test_the_dive_ends_feasible_where_the_rounding_is_stuck(seed):
    A, b, c, l, u, ints = mixed(40, 20, 10, seed)
    X = ref.lp_points(A, b, c, l, u, ints, 8, seed=seed)
    rounding = heur.round_repair_lift(A, b, c, l, u, ints, X)
    dive = ref.fix_propagate(A, b, c, l, u, ints, X, tol=1e-9)
    stuck = rounding[2] == heur.STUCK
    rescued = stuck & (dive['status'] == ref.FEASIBLE)
    print(seed, 'rounding', rounding[2].tolist(), 'dive', dive['status'].tolist(), 'tries', dive['counts'][:, 1].tolist())
    for k in np.flatnonzero(dive['status'] == ref.FEASIBLE):
        heur.certify(A, b, c, l, u, ints, dive['x'][k], dive['obj'][k])
        # ... and the heuristic's second pass leaves it feasible: no repair move, only lifts, no worse
        xt, obj, status, (repair, lift) = heur.round_repair_lift_one(A, b, c, l, u, ints, dive['x'][k])
        assert status == heur.FEASIBLE and repair == 0 and obj <= dive['obj'][k]
    assert (int(stuck.sum()), int(rescued.sum())) == COMPLEMENT[seed]
    assert rescued.sum() >= 1


# ---- the cases the GPU tests compare on ---------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(ref.CASES))
def test_cases_stay_clear_of_rounding_decisions(name):
    """On the restatement alone: at most 2 % of a case's points have a rounding decision within 1e-9 of flipping (the
    GPU test leaves those out of the comparison), and a capped case does cap."""
    A, b, c, l, u, ints, X, cutoff, max_tries, skip, want = ref.case(name)
    close = want['margin'] <= 1e-9
    print(name, 'cutoff', cutoff, 'status', np.bincount(want['status'], minlength=6).tolist(), 'close', int(close.sum()))
    assert close.sum() <= 0.02 * len(X)
    if 'tries' in name:
        assert np.any(want['status'] == ref.CAPPED) and np.all(want['counts'][want['status'] == ref.CAPPED, 1] == max_tries)
    if skip is not None:
        assert np.all(want['status'][skip == 1] == ref.SKIPPED) and np.isfinite(cutoff)


def test_cases_cover_every_status_and_shape():
    from tests.support.propagation_reference import SHAPES
    seen = np.zeros(6, np.int64)
    for name in ref.CASES:
        seen += np.bincount(ref.case(name)[-1]['status'], minlength=6)
    print(seen)
    assert np.all(seen[[ref.FEASIBLE, ref.STUCK, ref.CAPPED, ref.SKIPPED, ref.ROWS]] > 0)   # (INFEASIBLE_BOX: a test of its own)
    assert {(v[1], v[2]) for v in ref.CASES.values()} == set(SHAPES)
    assert {v[3] for v in ref.CASES.values()} >= {65} and {v[0] for v in ref.CASES.values()} == {'generator', 'mixed', 'half_continuous'}
