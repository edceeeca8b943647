"""The weighted row repair (include/mipx_wrepair.h), the parts that need no GPU: the header against the ctypes table
and the exported symbols, what BranchAndBound refuses at construction, the layout of the option's step buffer, and the
NumPy restatement of the algorithm (tests/support/weighted_repair_reference.py): its properties, and the condition on
the instances of the GPU tests that keeps those honest."""
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from simple_mip_solver_amd import BranchAndBound, PseudoCostBranchNode, _ffi
from tests.support import heuristic_reference as heur
from tests.support import weighted_repair_reference as ref
from tests.support.abi_check import agrees, prototypes
from tests.support.example_models import model
from tests.support.fix_propagate_reference import lp_points
from tests.support.propagation_reference import mixed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ['mipx_weighted_repair_batch', 'mipx_tree_set_weighted_repair', 'mipx_tree_weighted_repair_stats']


def test_weighted_repair_header_and_signature_table_agree():
    protos = prototypes('mipx_wrepair.h')
    assert sorted(protos) == sorted(_ffi.WREPAIR_SYMBOLS) == sorted(NAMES)
    for name, (ret, params) in protos.items():
        restype, argtypes = _ffi._WREPAIR_SIGNATURES[name]
        assert agrees(ret, restype), name
        assert len(params) == len(argtypes), name
        for k, (decl, ctype) in enumerate(zip(params, argtypes)):
            assert agrees(decl, ctype), f'{name} parameter {k} is `{decl}`, the table says {ctype}'


def test_new_symbols_overlap_no_existing_list():
    old = set(_ffi.SYMBOLS) | set(_ffi.SPILL_SYMBOLS) | set(_ffi.CUTMIG_SYMBOLS) | set(_ffi.DUALFN_SYMBOLS) | \
        set(_ffi.TREEREC_SYMBOLS) | set(_ffi.CGLP_SYMBOLS) | set(_ffi.RESTART_SYMBOLS) | set(_ffi.HEUR_SYMBOLS) | \
        set(_ffi.PROP_SYMBOLS) | set(_ffi.RCFIX_SYMBOLS) | set(_ffi.OBJSTEP_SYMBOLS) | set(_ffi.LSEARCH_SYMBOLS) | \
        set(_ffi.FIXPROP_SYMBOLS)
    assert not set(_ffi.WREPAIR_SYMBOLS) & old


def test_mipx_h_includes_the_header_and_keeps_its_version():
    text = open(os.path.join(ROOT, 'include', 'mipx.h')).read()
    assert '#include "mipx_wrepair.h"' in text
    assert _ffi.lib().mipx_abi_version() == 1


def test_library_exports_the_entries():
    L = _ffi.lib()
    for name in _ffi.WREPAIR_SYMBOLS:
        assert hasattr(L, name), name
        assert getattr(L, name).restype is _ffi._WREPAIR_SIGNATURES[name][0]


def test_stats_keys_and_status_codes_cover_the_header():
    text = open(os.path.join(ROOT, 'include', 'mipx_wrepair.h')).read()
    assert [int(k) for k in re.findall(r'\[(\d)\] ', text)] == list(range(8))
    assert _ffi.WREPAIR_STATS_KEYS == ('points', 'feasible', 'capped', 'moves', 'bumps', 'incumbents', 'reserved6', 'kernel_us')
    codes = {name.lower(): int(v) for name, v in re.findall(r'#define MIPX_WR_(\w+) (\d)', text)}
    assert codes == {v: k for k, v in _ffi.WREPAIR_STATUS.items()} and len(codes) == 3
    assert (ref.FEASIBLE, ref.CAPPED, ref.SKIPPED) == tuple(codes[k] for k in ('feasible', 'capped', 'skipped'))
    # the numbering is the heuristic's (there is no STUCK): the engine gates either kernel by the other's status
    assert all(_ffi.HEUR_STATUS[v] == k for k, v in codes.items()) and (heur.FEASIBLE, heur.CAPPED, heur.SKIPPED) == (0, 2, 3)
    assert _ffi.DEFAULT_WEIGHTED_REPAIR_STEPS == ref.MAX_STEPS == 256


def test_c_entries_refuse_null_arguments():
    L = _ffi.lib()
    assert L.mipx_weighted_repair_batch(None, 0, *([None] * 4), 0, 1e-9, 4, *([None] * 6)) == -1   # MIPX_EINVAL
    assert L.mipx_tree_set_weighted_repair(None, 4) == -1
    assert L.mipx_tree_weighted_repair_stats(None, None) == -1


def test_step_buffer_layout_matches_the_engine(tmp_path):
    cxx = os.environ.get('CXX') or shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.fail('no host C++ compiler (c++, g++ or clang++) to build the layout check with')
    exe = str(tmp_path / 'wr_layout_check')
    subprocess.run([cxx, '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror', '-I', os.path.join(ROOT, 'simple_mip_solver_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'support', 'wr_layout_check.cpp'), '-o', exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert ' 0 failed' in run.stdout, run.stdout


# ---- what the constructor refuses ------------------------------------------------------------------------------
def build(**extra):
    kw = dict(pseudo_costs={}, frontier_batch=4, gomory_cuts=False, primal_heuristic=True, weighted_repair=True)
    kw.update(extra)
    return BranchAndBound(model('small_branch'), PseudoCostBranchNode, **kw)


@pytest.mark.parametrize('value', [False, 0, -3, 2.5, 'on'])
def test_weighted_repair_value(value):
    with pytest.raises(AssertionError, match='weighted_repair is None, True or a positive number of steps'):
        build(weighted_repair=value)


def test_weighted_repair_needs_the_heuristic_and_refuses_the_dive():
    with pytest.raises(AssertionError, match='weighted_repair needs primal_heuristic'):
        build(primal_heuristic=None)
    with pytest.raises(AssertionError, match='weighted_repair cannot be combined with fix_propagate .*choose one'):
        build(fix_propagate=True)
    with pytest.raises(AssertionError, match='primal_heuristic needs frontier_batch'):
        build(frontier_batch=None)
    with pytest.raises(AssertionError, match='primal_heuristic needs gomory_cuts=False'):
        build(gomory_cuts=True)
    with pytest.raises(AssertionError, match='primal_heuristic cannot be combined with comm'):
        build(comm=object())


def test_option_is_off_by_default_and_inherited_by_restart():
    on = build()
    assert on._weighted_repair is True and on.weighted_repair_stats is None and on._given['weighted_repair'] is True
    assert build(weighted_repair=7)._given['weighted_repair'] == 7
    plain = build(weighted_repair=None)
    assert plain._weighted_repair is None and plain._given['weighted_repair'] is None and plain.weighted_repair_stats is None
    assert BranchAndBound(model('small_branch'), PseudoCostBranchNode, pseudo_costs={})._weighted_repair is None
    assert 'weighted_repair' in BranchAndBound._restart_overrides and 'primal_heuristic' in BranchAndBound._restart_overrides
    # (what it works beside)
    assert build(propagate=True, reduced_cost=True, objective_step=True, local_search=True, host_spill=1 << 24, dive=8,
                 anchor=False)._weighted_repair is True
    assert build(tree_record=True)._weighted_repair is True and build(dual_function=True)._weighted_repair is True
    assert build(weighted_repair=None, fix_propagate=True)._fix_propagate is True   # (the dive alone is as it was)


def test_restart_without_the_heuristic_drops_the_option(monkeypatch):
    from simple_mip_solver_amd.lp import CyLPArray
    src = build(tree_record=True, local_search=True)
    src.status = 'optimal'
    seeded = []
    monkeypatch.setattr(BranchAndBound, '_seed_native', lambda self, source: seeded.append(self))
    b = CyLPArray(np.asarray(src.root_node.lp.constraints[0].lower, dtype=np.float64).copy())
    new = src.restart(b, primal_heuristic=None)
    assert new._primal_heuristic is None and new._weighted_repair is None and new._local_search is None and seeded == [new]
    kept = src.restart(b)
    assert kept._primal_heuristic is True and kept._weighted_repair is True and kept._local_search is True
    fewer = src.restart(b, weighted_repair=3)
    assert fewer._weighted_repair == 3 and fewer._primal_heuristic is True
    off = src.restart(b, weighted_repair=None)
    assert off._weighted_repair is None and off._local_search is True
    swapped = src.restart(b, weighted_repair=None, fix_propagate=True)
    assert swapped._weighted_repair is None and swapped._fix_propagate is True
    with pytest.raises(AssertionError, match='weighted_repair needs primal_heuristic'):
        src.restart(b, primal_heuristic=None, weighted_repair=True)
    with pytest.raises(AssertionError, match='weighted_repair cannot be combined with fix_propagate'):
        src.restart(b, fix_propagate=True)


# ---- the restatement's properties --------------------------------------------------------------------------------
CONDITION = [(40, 20, 10, 0), (40, 20, 10, 1), (40, 20, 10, 2), (40, 20, 10, 3), (20, 10, 5, 0), (20, 10, 5, 1)]


@functools.lru_cache(maxsize=None)
def condition_case(args):
    """(instance, 64 LP points, the restatement's batch at cap 256, the rounding heuristic's batch) of mixed(*args)."""
    inst = mixed(*args)
    X = lp_points(*inst, 64, seed=args[3])
    return inst, X, ref.weighted_repair(*inst, X, max_steps=256), heur.round_repair_lift(*inst, X)


@pytest.mark.parametrize('args', CONDITION, ids=['mixed-%d-%d-%d-%d' % a for a in CONDITION])
def test_the_condition_that_keeps_the_gpu_tests_honest(args):
    """On 64 LP points of each instance, cap 256: the restatement ends FEASIBLE on all 64 and no point needs more than
    64 steps.  A restatement that does not is not the algorithm of the header."""
    inst, X, out, rounding = condition_case(args)
    steps = out['counts'].sum(axis=1)
    print(args, 'rounding feasible', int((rounding[2] == heur.FEASIBLE).sum()), 'weighted feasible', int((out['status'] == ref.FEASIBLE).sum()),
          'moves', out['counts'][:, 0].mean(), 'bumps', out['counts'][:, 1].mean(), 'max', out['counts'].max(axis=0).tolist(), 'steps', int(steps.max()))
    assert len(X) == 64 and np.all(out['status'] == ref.FEASIBLE)
    assert steps.max() <= 64


@pytest.mark.parametrize('args', CONDITION, ids=['mixed-%d-%d-%d-%d' % a for a in CONDITION])
def test_feasible_points_are_certified_and_rounding_feasible_points_are_the_round(args):
    (A, b, c, l, u, ints), X, out, rounding = condition_case(args)
    J = np.asarray(ints, dtype=np.int64)
    rest = np.setdiff1d(np.arange(A.shape[1]), J)
    for k in range(len(X)):
        assert out['status'][k] == ref.FEASIBLE
        heur.certify(A, b, c, l, u, ints, out['x'][k], out['obj'][k])
        assert np.array_equal(out['x'][k][rest], X[k][rest])   # (the other columns are unchanged)
        # a point whose ROUND already satisfies the rows: no move, no bump, and the point is the heuristic's ROUND
        xr, _, st, (repair, lift) = heur.round_repair_lift_one(A, b, c, l, u, ints, X[k], max_moves=0)
        if st == heur.FEASIBLE:
            assert (repair, lift) == (0, 0) and tuple(out['counts'][k]) == (0, 0)
            assert np.array_equal(out['x'][k].view(np.int64), xr.view(np.int64))
        else:
            assert out['counts'][k].sum() > 0


@pytest.mark.parametrize('args', CONDITION[:2] + CONDITION[4:5], ids=['mixed-%d-%d-%d-%d' % a for a in CONDITION[:2] + CONDITION[4:5]])
def test_with_the_weights_frozen_the_moves_are_the_heuristics_repair_moves(args):
    """Up to the first bump every weight is 1 and V is the heuristic's: the moves made until then are its repair moves.
    On a point the heuristic's repair mends (r moves), a cap of r gives its repaired point with r moves and no bump; on
    a point it is stuck on after r moves, the first r steps are those moves and step r + 1 is a bump."""
    (A, b, c, l, u, ints), X, out, rounding = condition_case(args)
    seen_mended = seen_stuck = 0
    for k in range(len(X)):
        r = int(rounding[3][k][0])
        trace = []
        ref.weighted_repair_one(A, b, c, l, u, ints, X[k], max_steps=256, trace=trace)
        xt = trace[0][1].copy()
        steps = trace[1:]
        first_bump = next((q for q, s in enumerate(steps) if s[0] == 'bump'), len(steps))
        for s in steps[:first_bump]:
            xt[s[1]] += s[2]
        if rounding[2][k] == heur.FEASIBLE:
            # (the heuristic with a cap of r makes its r repair moves and has none left for the lift)
            xh, _, st, (repair, lift) = heur.round_repair_lift_one(A, b, c, l, u, ints, X[k], max_moves=r)
            assert st == heur.FEASIBLE and (repair, lift) == (r, 0)
            xo, obj, status, counts = ref.weighted_repair_one(A, b, c, l, u, ints, X[k], max_steps=r)
            assert status == ref.FEASIBLE and counts == (r, 0) and first_bump == r == len(steps)
            assert np.array_equal(xo.view(np.int64), xh.view(np.int64)) and np.array_equal(xt.view(np.int64), xh.view(np.int64))
            seen_mended += r > 0
        else:
            assert rounding[2][k] == heur.STUCK and first_bump == r and len(steps) > r
            assert np.array_equal(xt.view(np.int64), rounding[0][k].view(np.int64))   # (the point the heuristic was stuck at)
            seen_stuck += 1
    assert seen_mended > 0 and seen_stuck > 0


def test_capped_returns_the_point_unchanged_and_counts_the_cap():
    (A, b, c, l, u, ints), X, out, _ = condition_case((40, 20, 10, 2))
    seen = 0
    for k in range(16):
        need = int(out['counts'][k].sum())
        for cap in {0, 1, need - 1} - {-1}:
            if cap >= need:
                continue
            xo, obj, status, counts = ref.weighted_repair_one(A, b, c, l, u, ints, X[k], max_steps=cap)
            assert status == ref.CAPPED and sum(counts) == cap and obj == 0.0
            assert np.array_equal(xo.view(np.int64), X[k].view(np.int64))
            seen += 1
        xo, _, status, counts = ref.weighted_repair_one(A, b, c, l, u, ints, X[k], max_steps=need)
        assert status == ref.FEASIBLE and sum(counts) == need   # (the cap is reached only while a row is violated)
    assert seen > 16


def test_restatement_edges():
    # x0 + x1 >= 3 and x0 + x1 <= 3 in 0..5 from (0.2, 0.4): both round to 0, V = 3; x0 up three times (ties: c, then column)
    A = np.array([[1.0, 1.0], [-1.0, -1.0]]); b = np.array([3.0, -3.0]); c = np.array([1.0, 2.0]); l = np.zeros(2); u = np.full(2, 5.0)
    xt, obj, status, counts = ref.weighted_repair_one(A, b, c, l, u, [0, 1], [0.2, 0.4])
    assert list(xt) == [3.0, 0.0] and obj == 3.0 and status == ref.FEASIBLE and counts == (3, 0)
    # a cover row and a pack row that a unit move trades one for one: x0 >= 1 (weight 1), -3 x0 >= -2 is broken by 1 when
    # x0 = 1 ... no point at all: only bumps and moves to and fro, to the cap
    A = np.array([[2.0], [-2.0]]); b = np.array([1.0, -1.0])
    xo, obj, status, counts = ref.weighted_repair_one(A, b, [1.0], [0.0], [5.0], [0], [0.4], max_steps=40)
    assert status == ref.CAPPED and sum(counts) == 40 and list(xo) == [0.4] and obj == 0.0
    # an integer column with l = u is no candidate: the other column does the work
    A = np.array([[1.0, 1.0]]); b = np.array([4.0])
    xt, obj, status, counts = ref.weighted_repair_one(A, b, [1.0, 5.0], [1.0, 0.0], [1.0, 9.0], [0, 1], [1.0, 0.3])
    assert list(xt) == [1.0, 3.0] and status == ref.FEASIBLE and counts == (3, 0)
    # ... and with no candidate at all every step is a bump
    xo, _, status, counts = ref.weighted_repair_one(A, b, [1.0, 5.0], [1.0, 0.0], [1.0, 0.0], [0, 1], [1.0, 0.0], max_steps=5)
    assert status == ref.CAPPED and counts == (0, 5)
    # fractional bounds are rounded as the heuristic rounds them; a continuous column is left alone
    xt, _, status, counts = ref.weighted_repair_one(np.zeros((0, 2)), [], [1.0, 1.0], [0.25, 0.0], [3.75, 1.0], [0], [0.0, 0.5])
    assert list(xt) == [1.0, 0.5] and status == ref.FEASIBLE and counts == (0, 0)
    # the batch: skip and gate
    A = np.array([[1.0]]); b = np.array([2.0])
    o = ref.weighted_repair(A, b, [1.0], [0.0], [5.0], [0], [[0.2]] * 5, skip=[1, 0, 0, 0, 0], gate=[1, 0, 1, 2, 3])
    assert list(o['status']) == [ref.SKIPPED, ref.SKIPPED, ref.FEASIBLE, ref.FEASIBLE, ref.SKIPPED]
    assert list(o['x'][:, 0]) == [0.2, 0.2, 2.0, 2.0, 0.2] and list(o['obj']) == [0.0, 0.0, 2.0, 2.0, 0.0]
    assert o['counts'].tolist() == [[0, 0], [0, 0], [2, 0], [2, 0], [0, 0]]


def test_a_bump_is_what_gets_a_stuck_point_moving():
    """Two rows side by side that one unit move trades against each other: 3 x0 >= 3 is short by 3 at x0 = 0, and
    -4 x0 >= -2 ... the move up mends 3 and breaks 2: it is taken at once.  Turned round (mends 2, breaks 3) it needs
    the weight of the violated row to reach 2 first."""
    A = np.array([[2.0, 0.0], [-3.0, 1.0]]); b = np.array([2.0, 0.0]); c = np.array([1.0, 1.0]); l = np.zeros(2); u = np.full(2, 9.0)
    # from (0, 0): s = (-2, 0), V = 2.  x0 up gives s = (0, -3), V' = 3; x1 up changes nothing of row 0, V' = 2: no V' < V
    assert heur.round_repair_lift_one(A, b, c, l, u, [0, 1], [0.0, 0.0])[2] == heur.STUCK
    trace = []
    xt, obj, status, counts = ref.weighted_repair_one(A, b, c, l, u, [0, 1], [0.0, 0.0], trace=trace)
    assert status == ref.FEASIBLE and list(xt) == [1.0, 3.0] and counts == (4, 1)
    assert [s[0] for s in trace[1:]] == ['bump', 'move', 'move', 'move', 'move'] and trace[2] == ('move', 0, 1.0)
    heur.certify(A, b, c, l, u, [0, 1], xt, obj)



# ---- the cases the GPU tests compare on ---------------------------------------------------------------------------
def test_cases_cover_every_status_path_and_shape():
    seen = np.zeros(4, np.int64)
    bumps_with_several_columns_per_thread = 0
    for name, spec in ref.CASES.items():
        A, b, c, l, u, ints, X, max_steps, tol, skip, gate, want = ref.case(name)
        seen += np.bincount(want['status'], minlength=4)
        assert A.shape == (spec[2], spec[1]) and len(X) == spec[3]
        if 'steps' in name:   # (a capped case does cap, at the cap)
            capped = want['status'] == ref.CAPPED
            assert capped.any() and np.all(want['counts'][capped].sum(axis=1) == max_steps)
        if skip is not None:
            assert np.all(want['status'][skip == 1] == ref.SKIPPED)
        if gate is not None:
            assert np.all(want['status'][(gate == 0) | (gate == 3)] == ref.SKIPPED) and np.any(want['status'][gate == 1] != ref.SKIPPED)
        if 'fixed' in name:
            assert np.all(u[ints[::7]] == l[ints[::7]]) and np.all(want['x'][:, ints[::7]] == l[ints[::7]])
        if len(ints) > 256:
            bumps_with_several_columns_per_thread += int(want['counts'][:, 1].sum())
    print(seen, bumps_with_several_columns_per_thread)
    assert seen[ref.FEASIBLE] > 300 and seen[ref.CAPPED] > 10 and seen[ref.SKIPPED] > 50 and seen[1] == 0
    assert bumps_with_several_columns_per_thread > 0
    assert {(v[1], v[2]) for v in ref.CASES.values()} == {(8, 4), (40, 20), (70, 33), (64, 300), (300, 150), (1000, 700)}
    assert {v[3] for v in ref.CASES.values()} >= {3, 65} and {v[0] for v in ref.CASES.values()} == {'generator', 'mixed', 'half_continuous'}
