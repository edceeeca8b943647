"""The LP dive (include/mipx_lpdive.h), the parts that need no GPU: the header against the ctypes table and the exported
symbols, what BranchAndBound refuses at construction, and the NumPy restatement of the algorithm
(tests/support/lp_dive_reference.py) around the oracle's node LP: its edge cases, its points judged by scipy (linprog on
the same fixed integers, milp for the optimum), and the figure the option was proposed with."""
import functools
import os
import re

import numpy as np
import pytest
from scipy.optimize import Bounds, LinearConstraint, linprog, milp

from simple_mip_solver_amd import BranchAndBound, PseudoCostBranchNode, _ffi
from tests.support import completion_reference as comp
from tests.support import heuristic_reference as heur
from tests.support import lp_dive_reference as ref
from tests.support.abi_check import agrees, prototypes
from tests.support.example_models import model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ['mipx_lpdive_batch', 'mipx_tree_set_lpdive', 'mipx_tree_lpdive_stats']


def test_lp_dive_header_and_signature_table_agree():
    protos = prototypes('mipx_lpdive.h')
    assert sorted(protos) == sorted(_ffi.LPDIVE_SYMBOLS) == sorted(NAMES)
    for name, (ret, params) in protos.items():
        restype, argtypes = _ffi._LPDIVE_SIGNATURES[name]
        assert agrees(ret, restype), name
        assert len(params) == len(argtypes), name
        for k, (decl, ctype) in enumerate(zip(params, argtypes)):
            assert agrees(decl, ctype), f'{name} parameter {k} is `{decl}`, the table says {ctype}'
    assert len(protos['mipx_lpdive_batch'][1]) == 19


def test_new_symbols_overlap_no_existing_list():
    old = set(_ffi.SYMBOLS) | set(_ffi.SPILL_SYMBOLS) | set(_ffi.CUTMIG_SYMBOLS) | set(_ffi.DUALFN_SYMBOLS) | \
        set(_ffi.TREEREC_SYMBOLS) | set(_ffi.CGLP_SYMBOLS) | set(_ffi.RESTART_SYMBOLS) | set(_ffi.HEUR_SYMBOLS) | \
        set(_ffi.PROP_SYMBOLS) | set(_ffi.RCFIX_SYMBOLS) | set(_ffi.OBJSTEP_SYMBOLS) | set(_ffi.LSEARCH_SYMBOLS) | \
        set(_ffi.FIXPROP_SYMBOLS) | set(_ffi.WREPAIR_SYMBOLS) | set(_ffi.CUBE_SYMBOLS) | set(_ffi.COMPLETE_SYMBOLS) | \
        set(_ffi.FINISH_SYMBOLS)
    assert not set(_ffi.LPDIVE_SYMBOLS) & old
    assert 'mipx_lp_dive_batch' in _ffi.SYMBOLS   # (the in-place plunge's entry: another name, untouched)
    assert len(_ffi._SIGNATURES) == 70   # (the new entries have a table of their own)


def test_mipx_h_includes_the_header_and_declares_nothing_new_itself():
    text = open(os.path.join(ROOT, 'include', 'mipx.h')).read()
    assert '#include "mipx_lpdive.h"' in text
    assert 'lpdive' not in re.sub(r'#include "mipx_lpdive.h".*', '', text)
    assert _ffi.lib().mipx_abi_version() == 1


def test_library_exports_the_entries():
    L = _ffi.lib()
    for name in _ffi.LPDIVE_SYMBOLS:
        assert hasattr(L, name), name
        assert getattr(L, name).restype is _ffi._LPDIVE_SIGNATURES[name][0]


def test_stats_keys_and_status_codes_cover_the_header():
    text = open(os.path.join(ROOT, 'include', 'mipx_lpdive.h')).read()
    assert [int(k) for k in re.findall(r'\[(\d)\] ', text)] == list(range(8))
    assert _ffi.LPDIVE_STATS_KEYS == ('points', 'feasible', 'infeasible', 'failed', 'moves', 'incumbents', 'pivots', 'kernel_us')
    codes = {name.lower(): int(v) for name, v in
             re.findall(r'#define MIPX_LPDIVE_(FEASIBLE|INFEASIBLE|LIMIT|SKIPPED|REJECTED|CUTOFF) (\d)', text)}
    assert codes == {v: k for k, v in _ffi.LPDIVE_STATUS.items()} and len(codes) == 6
    assert (ref.FEASIBLE, ref.INFEASIBLE, ref.LIMIT, ref.SKIPPED, ref.REJECTED, ref.CUTOFF) == \
        tuple(codes[k] for k in ('feasible', 'infeasible', 'limit', 'skipped', 'rejected', 'cutoff'))
    # FEASIBLE and SKIPPED are the heuristic's feasible and skipped, as in the other families
    assert _ffi.HEUR_STATUS[codes['feasible']] == 'feasible' and _ffi.HEUR_STATUS[codes['skipped']] == 'skipped'
    assert _ffi.COMPLETE_STATUS[codes['feasible']] == 'completed' and _ffi.COMPLETE_STATUS[codes['skipped']] == 'skipped'
    rules = dict(re.findall(r'#define MIPX_LPDIVE_RULE_(FRACTIONAL|COEFFICIENT) (\d)', text))
    assert {k.lower(): int(v) for k, v in rules.items()} == _ffi.LPDIVE_RULES == dict(fractional=ref.FRACTIONAL, coefficient=ref.COEFFICIENT)
    assert int(re.search(r'#define MIPX_LPDIVE_MAX_ROUNDS (\d+)', text).group(1)) == _ffi.MAX_LP_DIVE_ROUNDS == 1024
    assert _ffi.DEFAULT_LP_DIVE_ROUNDS == 64 and ref.FTOL == ref.CTOL == 1e-6


def test_c_entries_refuse_null_arguments():
    L = _ffi.lib()
    assert L.mipx_lpdive_batch(None, 0, *([None] * 4), 0, None, None, np.inf, 1, 0, *([None] * 7)) == -1   # MIPX_EINVAL
    assert L.mipx_tree_set_lpdive(None, 64, 0, 0) == -1
    assert L.mipx_tree_lpdive_stats(None, None) == -1


# ---- what the constructor refuses ------------------------------------------------------------------------------
def build(**extra):
    kw = dict(pseudo_costs={}, frontier_batch=4, gomory_cuts=False, primal_heuristic=True, lp_dive=True)
    kw.update(extra)
    return BranchAndBound(model('small_branch'), PseudoCostBranchNode, **kw)


@pytest.mark.parametrize('value', [False, 0, 1025, -1, 2.5, 'on'])
def test_lp_dive_value(value):
    with pytest.raises(ValueError, match='lp_dive is None, True or a round cap from 1 to 1024'):
        build(lp_dive=value)


@pytest.mark.parametrize('value', [False, True, 0, -3, 2.5, 'on'])
def test_lp_dive_every_value(value):
    with pytest.raises(ValueError, match='lp_dive_every is None or a positive integer'):
        build(lp_dive_every=value)


def test_lp_dive_needs_the_heuristic():
    with pytest.raises(ValueError, match='lp_dive needs primal_heuristic'):
        build(primal_heuristic=None)
    with pytest.raises(ValueError, match='lp_dive_every needs lp_dive'):
        build(lp_dive=None, lp_dive_every=2)
    with pytest.raises(AssertionError, match='primal_heuristic needs frontier_batch'):
        build(frontier_batch=None)
    with pytest.raises(AssertionError, match='primal_heuristic needs gomory_cuts=False'):
        build(gomory_cuts=True)
    with pytest.raises(AssertionError, match='primal_heuristic cannot be combined with comm'):
        build(comm=object())


def test_option_is_off_by_default_and_works_beside_the_others():
    on = build()
    assert on._lp_dive is True and on._lp_dive_every is None and on.lp_dive_stats is None and on._given['lp_dive'] is True
    assert build(lp_dive=1)._lp_dive == 1 and build(lp_dive=1024, lp_dive_every=5)._lp_dive_every == 5
    plain = build(lp_dive=None)
    assert plain._lp_dive is None and plain._given['lp_dive'] is None and plain.lp_dive_stats is None
    assert BranchAndBound(model('small_branch'), PseudoCostBranchNode, pseudo_costs={})._lp_dive is None
    assert 'lp_dive' in BranchAndBound._restart_overrides and 'lp_dive_every' in BranchAndBound._restart_overrides
    assert build(propagate=True, reduced_cost=True, objective_step=True, local_search=True, host_spill=1 << 24, dive=8,
                 anchor=False)._lp_dive is True
    assert build(tree_record=True)._lp_dive is True and build(dual_function=True)._lp_dive is True
    assert build(fix_propagate=True, cube_search=True, complete_continuous=True)._lp_dive is True
    assert build(weighted_repair=True, cube_search=7, local_search=True, complete_continuous=True)._lp_dive is True


def test_restart_inherits_the_option_and_drops_it_with_the_heuristic(monkeypatch):
    from simple_mip_solver_amd.lp import CyLPArray
    src = build(tree_record=True, lp_dive=32, lp_dive_every=4)
    src.status = 'optimal'
    seeded = []
    monkeypatch.setattr(BranchAndBound, '_seed_native', lambda self, source: seeded.append(self))
    b = CyLPArray(np.asarray(src.root_node.lp.constraints[0].lower, dtype=np.float64).copy())
    kept = src.restart(b)
    assert kept._lp_dive == 32 and kept._lp_dive_every == 4 and kept._primal_heuristic is True
    new = src.restart(b, primal_heuristic=None)
    assert new._primal_heuristic is None and new._lp_dive is None and new._lp_dive_every is None and seeded == [kept, new]
    off = src.restart(b, lp_dive=None)
    assert off._lp_dive is None and off._lp_dive_every is None and off._primal_heuristic is True
    assert src.restart(b, lp_dive=True, lp_dive_every=None)._lp_dive is True
    with pytest.raises(ValueError, match='lp_dive needs primal_heuristic'):
        src.restart(b, primal_heuristic=None, lp_dive=True)


# ---- the restatement around the oracle's node LP: edge cases ----------------------------------------------------------
def small():
    """min x0 + 2 x1, 1.25 <= x0 + x1 <= 3, 0 <= x0 <= 5, 0 <= x1: the LP optimum is (1.25, 0)."""
    A = np.array([[1.0, 1.0], [-1.0, -1.0]]); b = np.array([1.25, -3.0]); c = np.array([1.0, 2.0])
    return A, b, c, np.zeros(2), np.array([5.0, np.inf])


def test_restatement_one_integer_column_and_an_infinite_upper_bound():
    A, b, c, l, u = small()
    lp = ref.oracle_lp(A, b, c)
    x0 = lp(l[None], u[None], np.zeros((1, 4), np.int8))
    assert x0['status'][0] == 0 and list(x0['x'][0]) == [1.25, 0.0]
    # n_int = 1, a continuous column with u = +inf: x0 is fixed at 1, the LP moves x1 to 0.25; then FINAL and FINISH
    o = ref.dive(A, b, c, l, u, [0], x0['x'], lp, vstat=x0['vstat'])
    assert o['status'][0] == ref.FEASIBLE and list(o['x'][0]) == [1.0, 0.25] and o['obj'][0] == 1.5
    assert (o['rounds'][0], o['fixings'][0], o['flips'][0]) == (2, 1, 0)
    cold = ref.dive(A, b, c, l, u, [0], x0['x'], lp)
    assert cold['status'][0] == ref.FEASIBLE and list(cold['x'][0]) == [1.0, 0.25]
    # the round cap: one LP is not enough (the FINAL LP would be the second), two are
    o = ref.dive(A, b, c, l, u, [0], x0['x'], lp, max_rounds=1)
    assert o['status'][0] == ref.LIMIT and list(o['x'][0]) == [1.25, 0.0] and o['obj'][0] == 0.0 and o['rounds'][0] == 1
    assert ref.dive(A, b, c, l, u, [0], x0['x'], lp, max_rounds=2)['status'][0] == ref.FEASIBLE
    # an integral point goes straight to FINAL: one LP
    o = ref.dive(A, b, c, l, u, [0], [[2.0, 0.0]], lp, max_rounds=1)
    assert o['status'][0] == ref.FEASIBLE and list(o['x'][0]) == [2.0, 0.0] and (o['rounds'][0], o['fixings'][0]) == (1, 0)


def test_restatement_both_rules():
    A, b, c, l, u = small()
    A1, b1 = A[:1], b[:1]   # (the covering row alone: lowering a column can break it, raising cannot)
    lp = ref.oracle_lp(A1, b1, c)
    assert [list(v) for v in ref.locks(A1, [0, 1])] == [[1, 1], [0, 0]] and [list(v) for v in ref.locks(A, [0])] == [[1], [1]]
    near = ref.dive(A1, b1, c, l, u, [0], [[1.25, 0.0]], lp, rule=ref.FRACTIONAL)
    up = ref.dive(A1, b1, c, l, u, [0], [[1.25, 0.0]], lp, rule=ref.COEFFICIENT)
    assert list(near['x'][0]) == [1.0, 0.25] and near['obj'][0] == 1.5      # (to the nearest)
    assert list(up['x'][0]) == [2.0, 0.0] and up['obj'][0] == 2.0           # (up_j = 0 < down_j = 1: up)
    # a tie of the lock counts rounds to the nearest
    tie = ref.dive(A, b, c, l, u, [0], [[1.25, 0.0]], ref.oracle_lp(A, b, c), rule=ref.COEFFICIENT)
    assert list(tie['x'][0]) == [1.0, 0.25]


def test_restatement_every_column_integer():
    A, b, c, l, u = small()
    u2 = np.array([5.0, 5.0])
    lp = ref.oracle_lp(A, b, c)
    # n_int = n: x0 = 1.25 is fixed at 1; the LP puts x1 at 0.25; x1 is fixed at 0: infeasible; flipped to [1, 5]: (1, 1)
    o = ref.dive(A, b, c, l, u2, [0, 1], [[1.25, 0.0]], lp)
    assert o['status'][0] == ref.FEASIBLE and list(o['x'][0]) == [1.0, 1.0] and o['obj'][0] == 3.0
    assert (o['fixings'][0], o['flips'][0]) == (2, 1) and o['rounds'][0] == 4


def test_restatement_flip_into_an_empty_range_and_infeasible_without_a_fixing():
    A = np.array([[1.0, 1.0]]); b = np.array([1.5]); c = np.array([1.0, 2.0])
    l = np.zeros(2); u = np.array([3.0, 1.0])
    lp = ref.oracle_lp(A, b, c)
    # a point below its box: x0 = -0.5 is fixed at 0 (clipped), the LP needs x1 >= 1.5 > 1: infeasible; the flip's
    # range [0, -1] is empty
    o = ref.dive(A, b, c, l, u, [0], [[-0.5, 1.0]], lp)
    assert o['status'][0] == ref.INFEASIBLE and list(o['x'][0]) == [-0.5, 1.0] and (o['fixings'][0], o['flips'][0], o['rounds'][0]) == (1, 0, 1)
    # FINAL's LP infeasible: no fixing is on record
    o = ref.dive(A, b, c, l, u, [0], [[0.0, 1.0]], lp)
    assert o['status'][0] == ref.INFEASIBLE and (o['fixings'][0], o['flips'][0], o['rounds'][0]) == (0, 0, 1)
    # a flip that helps: 0.4 -> 0 is infeasible, flipped to [1, 3] the LP gives (1.5, 0); 1.5 -> floor(2.0) = 2: (2, 0)
    o = ref.dive(A, b, c, l, u, [0], [[0.4, 1.0]], lp)
    assert o['status'][0] == ref.FEASIBLE and list(o['x'][0]) == [2.0, 0.0] and o['obj'][0] == 2.0
    assert (o['fixings'][0], o['flips'][0], o['rounds'][0]) == (2, 1, 4)


def test_restatement_cutoff_and_skipped_points():
    A, b, c, l, u = small()
    lp = ref.oracle_lp(A, b, c)
    X = np.array([[1.25, 0.0]] * 5)
    X[3, 1] = np.nan
    L, U = np.tile(l, (5, 1)), np.tile(u, (5, 1))
    L[1, 0] = 0.5        # an integer column with a fractional bound
    U[2, 0] = np.inf     # ... with an infinite one
    o = ref.dive(A, b, c, L, U, [0], X, lp, skip=[0, 0, 0, 0, 1])
    assert list(o['status']) == [ref.FEASIBLE] + [ref.SKIPPED] * 4
    assert not o['rounds'][1:].any() and not o['pivots'][1:].any() and not o['obj'][1:].any()
    assert np.array_equal(o['x'][1:].view(np.int64), X[1:].view(np.int64))
    # a bound within ctol of an integer is that integer
    L[1, 0] = 3e-7
    assert ref.dive(A, b, c, L, U, [0], X, lp)['status'][1] == ref.FEASIBLE
    # the first LP's objective is 1.5: a cutoff at or below it ends the dive there, one above lets it finish
    assert ref.dive(A, b, c, l, u, [0], X[:1], lp, cutoff=1.5)['status'][0] == ref.CUTOFF
    o = ref.dive(A, b, c, l, u, [0], X[:1], lp, cutoff=1.0)
    assert o['status'][0] == ref.CUTOFF and o['rounds'][0] == 1 and list(o['x'][0]) == [1.25, 0.0] and o['obj'][0] == 0.0
    assert ref.dive(A, b, c, l, u, [0], X[:1], lp, cutoff=1.5 + 1e-9)['status'][0] == ref.FEASIBLE
    assert len(ref.dive(A, b, c, l, u, [0], np.zeros((0, 2)), lp)['status']) == 0
    # an LP function that calls a wrong point optimal is caught: REJECTED, the point unchanged
    liar = lambda Lk, Uk, Vk: dict(status=np.zeros(1, np.int32), obj=np.zeros(1), x=np.array([[1.0, 0.0]]),   # noqa: E731
                                   vstat=np.zeros((1, 4), np.int8), npivots=np.ones(1, np.int32))
    o = ref.dive(A, b, c, l, u, [0], X[:1], liar)
    assert o['status'][0] == ref.REJECTED and list(o['x'][0]) == [1.25, 0.0] and o['obj'][0] == 0.0 and o['pivots'][0] == 2


# ---- the restatement judged by scipy -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def run(family, seed):
    """(instance, points, codes, boxes, the completion's batch, the dive's by either rule) at 40 x 20, made once."""
    inst = getattr(comp, family)(40, 20, seed)
    A, b, c, l, u, ints = inst
    X, V, L, U = ref.profile_points(inst, seed, 64)
    Xt = heur.round_repair_lift(A, b, c, l, u, ints, X)[0]
    done = comp.complete(A, b, c, l, u, ints, Xt, comp.oracle_lp(A, b, c), vstat=V)
    lp = ref.oracle_lp(A, b, c)
    return inst, X, V, L, U, done, [ref.dive(A, b, c, L, U, ints, X, lp, vstat=V, rule=rule) for rule in (0, 1)]


@functools.lru_cache(maxsize=None)
def milp_optimum(family, seed):
    A, b, c, l, u, ints = getattr(comp, family)(40, 20, seed)
    integrality = np.zeros(len(c))
    integrality[ints] = 1
    h = milp(c, constraints=LinearConstraint(A, lb=b, ub=np.inf), bounds=Bounds(l, u), integrality=integrality,
             options={'mip_rel_gap': 0.0})
    assert h.status == 0
    return float(h.fun)


@pytest.mark.parametrize('seed', [0, 1, 2, 3])
@pytest.mark.parametrize('family', ['mixed', 'packing'])
def test_feasible_points_are_valid_with_milp_as_the_judge(family, seed):
    (A, b, c, l, u, ints), X, V, L, U, done, dives = run(family, seed)
    best = milp_optimum(family, seed)
    for rule, o in enumerate(dives):
        print(family, seed, 'rule', rule, 'status', np.bincount(o['status'], minlength=6), 'completion', int((done['status'] == 0).sum()),
              'rounds', o['rounds'].max(), 'best', o['obj'][o['status'] == 0].min() if (o['status'] == 0).any() else None, 'milp', best)
        assert set(o['status']) <= {ref.FEASIBLE, ref.INFEASIBLE}   # (64 rounds are enough at 20 integer columns; no LP at its limit)
        for p in np.flatnonzero(o['status'] == ref.FEASIBLE):
            x = o['x'][p]
            assert np.all(A @ x - b >= -1e-6) and np.all(x >= L[p] - 1e-6) and np.all(x <= U[p] + 1e-6)
            assert np.array_equal(x[ints], np.rint(x[ints]))
            lo, hi = L[p].copy(), U[p].copy()
            lo[ints] = x[ints]
            hi[ints] = x[ints]
            h = linprog(c, A_ub=-A, b_ub=-b, bounds=list(zip(lo, hi)), method='highs')
            assert h.status == 0 and abs(o['obj'][p] - h.fun) <= 1e-9 * max(1.0, abs(h.fun)), (p, o['obj'][p], h.fun)
            assert o['obj'][p] >= best - 1e-9 * max(1.0, abs(best))
        rest = o['status'] != ref.FEASIBLE
        assert np.array_equal(o['x'][rest].view(np.int64), X[rest].view(np.int64)) and not o['obj'][rest].any()


def test_the_figure_of_the_issue_at_mixed_40_by_20_seed_1():
    """Mixed 40 x 20, seed 1, 64 LP points by the recipe of scripts/completion_profile.py, each dived inside its own node
    box: rounding and completing all integers at once ends feasible on none of them, the dive on some.  The CPU loop the
    option was proposed with gave 25 of 64; this restatement (the flip in a round of its own, a final LP) gives 25 too,
    by either rule."""
    inst, X, V, L, U, done, dives = run('mixed', 1)
    counts = [int((o['status'] == ref.FEASIBLE).sum()) for o in dives]
    print('completion', int((done['status'] == comp.COMPLETED).sum()), 'dive', counts, 'flips', [int(o['flips'].sum()) for o in dives])
    assert int((done['status'] == comp.COMPLETED).sum()) == 0
    assert min(counts) >= 1
    assert all(o['flips'].sum() > 0 for o in dives)
