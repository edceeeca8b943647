"""Lifted cover cuts in the native search (BranchAndBound(root_cuts=..., cover_cuts=True), include/mipx_cover.h) on the
sparse knapsack family: the search with the option against the search without it and scipy's milp (HiGHS), the cuts
it keeps against HiGHS, the option beside the other options of the native search, a family of general integers on
which it finds nothing, and what the constructor refuses."""
import functools

import numpy as np
import pytest
from scipy.optimize import Bounds, LinearConstraint, milp

from simple_mip_solver_amd import BranchAndBound, MILPInstance, PseudoCostBranchDepthFirstSearchNode, PseudoCostBranchNode
from simple_mip_solver_amd.generators import random_dense_milp_arrays, sparse_knapsack_milp_arrays

pytestmark = pytest.mark.gpu
CASES = [(16, 8, 6, seed) for seed in range(4)] + [(40, 20, 8, seed) for seed in range(2)]
DENSE = ('dense', 20, 10, 1)
COVER_STATS = ['rounds', 'rows', 'found', 'skipped', 'selected', 'kept', 'kernel_us']
STATS = ['rounds', 'base_rows', 'found', 'selected', 'kept', 'bound_before', 'bound_after', 'lp_pivots', 'kernel_us']


def arrays(case):
    if case[0] == 'dense':
        return random_dense_milp_arrays(case[1], case[2], seed=case[3])
    return sparse_knapsack_milp_arrays(*case[:3], seed=case[3])


@functools.lru_cache(maxsize=None)
def highs_optimum(case):
    A, b, c, l, u, ints = arrays(case)
    h = milp(c, constraints=LinearConstraint(A, lb=b, ub=np.inf), bounds=Bounds(l, u), integrality=np.ones(len(c)),
             options={'mip_rel_gap': 0.0})
    assert h.status == 0
    return float(h.fun)


def search(case, Node=PseudoCostBranchNode, **kw):
    A, b, c, l, u, ints = arrays(case)
    mdl = MILPInstance(A=A, b=b, c=c, l=l, u=u, sense=['Min', '>='], integerIndices=ints, numVars=len(c))
    bb = BranchAndBound(mdl, Node, pseudo_costs={}, gomory_cuts=False, mip_gap=0.0, frontier_batch=64, **kw)
    bb.solve()
    return bb


@functools.lru_cache(maxsize=None)
def plain(case):
    bb = search(case)
    assert bb.root_cut_stats is None and bb.root_cuts is None and bb.cover_cut_stats is None
    return bb.status, float(bb.objective_value), bb.evaluated_nodes


@functools.lru_cache(maxsize=None)
def with_covers(case):
    return search(case, root_cuts=True, cover_cuts=True)


def close(a, b):
    """tests/test_root_cuts_gpu.py's comparison of two optima: 1e-6 relative."""
    return abs(a - b) <= 1e-6 * max(1.0, abs(b))


def assert_optimal(bb, case):
    A, b, c, l, u, ints = arrays(case)
    assert bb.status == 'optimal' == plain(case)[0]
    print(case, bb.objective_value, plain(case)[1], highs_optimum(case), 'nodes', bb.evaluated_nodes, plain(case)[2],
          bb.root_cut_stats, bb.cover_cut_stats)
    assert close(bb.objective_value, plain(case)[1]) and close(bb.objective_value, highs_optimum(case))
    x = np.asarray(bb.solution, dtype=np.float64)
    assert x.shape == (len(c),) and close(float(c @ x), bb.objective_value)
    assert np.all(A @ x >= b - 1e-6) and np.all(x >= l - 1e-9) and np.all(x <= u + 1e-9)
    assert np.all(np.abs(x - np.round(x)) <= 1e-4)
    assert bb.model.A.shape == A.shape   # (the model is the one given: the cut rows live in the engine's problem)


@pytest.mark.parametrize('case', CASES, ids=str)
def test_search_with_cover_cuts_finds_the_same_optimum(case):
    bb = with_covers(case)
    assert_optimal(bb, case)
    st, cs = bb.root_cut_stats, bb.cover_cut_stats
    assert list(st) == STATS and list(cs) == COVER_STATS
    assert cs['found'] >= 1 and cs['kept'] <= cs['selected'] <= cs['found']
    assert cs['rounds'] == st['rounds'] >= 1 and cs['rows'] == cs['rounds'] * case[1] and cs['skipped'] == 0
    assert cs['kernel_us'] > 0 and st['kept'] <= st['selected'] <= st['found']
    assert st['kept'] + cs['kept'] == len(bb.root_cuts) <= 64
    assert st['bound_after'] >= st['bound_before'] - 1e-9 * abs(st['bound_before'])
    A, b, c, l, u, ints = arrays(case)
    x = np.asarray(bb.solution, dtype=np.float64)
    for pi, pi0 in bb.root_cuts:
        assert pi.shape == (case[0],) and np.isfinite(pi0)
        assert float(pi @ x) >= pi0 - 1e-6 * (abs(pi0) + float(np.abs(pi) @ np.abs(x)))   # (the optimum is not cut off)


@pytest.mark.parametrize('case', CASES, ids=str)
def test_every_kept_cut_is_valid_by_highs(case):
    A, b, c, l, u, ints = arrays(case)
    for pi, pi0 in with_covers(case).root_cuts:
        h = milp(pi, constraints=LinearConstraint(A, lb=b, ub=np.inf), bounds=Bounds(l, u), integrality=np.ones(len(c)),
                 options={'mip_rel_gap': 0.0})
        assert h.status == 0
        assert float(h.fun) >= pi0 - 1e-6 * (abs(pi0) + float(np.abs(pi) @ np.maximum(np.abs(l), np.abs(u)))), (h.fun, pi0)


def test_cover_cuts_are_kept_and_gain_bound():
    kept = [with_covers(case).cover_cut_stats['kept'] for case in CASES]
    gain = [with_covers(case).root_cut_stats['bound_after'] - with_covers(case).root_cut_stats['bound_before'] for case in CASES]
    print(kept, gain)
    assert sum(kept) >= 1 and max(gain) > 1e-6


@pytest.mark.parametrize('case', [(16, 8, 6, 1), (40, 20, 8, 0)], ids=str)
def test_cover_cuts_beside_the_other_options(case):
    bb = search(case, root_cuts=True, cover_cuts=True, primal_heuristic=True, objective_step=True, reduced_cost=True,
                propagate=True)
    assert_optimal(bb, case)
    assert bb.heuristic_stats is not None and bb.cover_cut_stats['found'] >= 1
    bb = search(case, Node=PseudoCostBranchDepthFirstSearchNode, root_cuts=3, root_cut_rows=8, cover_cuts=True,
                primal_heuristic=True)
    assert_optimal(bb, case)
    assert bb.cover_cut_stats['rounds'] <= 3 and len(bb.root_cuts) <= 8 and bb.cover_cut_stats['found'] >= 1


def test_general_integers_give_no_cover_and_the_same_search():
    mir = search(DENSE, root_cuts=True)
    bb = search(DENSE, root_cuts=True, cover_cuts=True)
    cs = bb.cover_cut_stats
    assert cs['found'] == cs['selected'] == cs['kept'] == cs['skipped'] == 0 and cs['rounds'] == bb.root_cut_stats['rounds']
    assert (bb.status, float(bb.objective_value), bb.evaluated_nodes) == \
        (mir.status, float(mir.objective_value), mir.evaluated_nodes)
    assert len(bb.root_cuts) == len(mir.root_cuts) and all(
        np.array_equal(p, q) and p0 == q0 for (p, p0), (q, q0) in zip(bb.root_cuts, mir.root_cuts))
    assert mir.cover_cut_stats is None and close(bb.objective_value, highs_optimum(DENSE))


def test_the_option_off_changes_nothing():
    case = (16, 8, 6, 2)
    bb = search(case, cover_cuts=None)
    assert bb.cover_cut_stats is None and bb.root_cuts is None
    assert (bb.status, float(bb.objective_value), bb.evaluated_nodes) == plain(case)
    bb = search(case, root_cuts=True)
    assert bb.cover_cut_stats is None and list(bb.root_cut_stats) == STATS
    assert bb.root_cut_stats['kept'] == len(bb.root_cuts)


def test_refused_combinations():
    A, b, c, l, u, ints = arrays((16, 8, 6, 0))
    mdl = MILPInstance(A=A, b=b, c=c, l=l, u=u, sense=['Min', '>='], integerIndices=ints, numVars=len(c))

    def make(**kw):
        kw.setdefault('gomory_cuts', False)
        return BranchAndBound(mdl, PseudoCostBranchNode, pseudo_costs={}, **kw)

    with pytest.raises(AssertionError, match='cover_cuts needs root_cuts'):
        make(frontier_batch=64, cover_cuts=True)
    for bad in (False, 1, 3, 'yes'):
        with pytest.raises(AssertionError, match='cover_cuts is None or True'):
            make(frontier_batch=64, root_cuts=True, cover_cuts=bad)
    with pytest.raises(AssertionError, match='root_cuts needs frontier_batch'):
        make(root_cuts=True, cover_cuts=True)
    bb = make(frontier_batch=64, root_cuts=True, cover_cuts=True)
    assert bb._cover_cuts is True and bb.cover_cut_stats is None
