"""Root MIR cuts in the native search (BranchAndBound(root_cuts=...), include/mipx_mir.h): the search with the option
against the search without it and scipy's milp (HiGHS), the cuts it keeps against HiGHS, the option beside the other
options of the native search, and what the constructor refuses."""
import functools

import numpy as np
import pytest
from scipy.optimize import Bounds, LinearConstraint, milp

from simple_mip_solver_amd import BranchAndBound, MILPInstance, PseudoCostBranchDepthFirstSearchNode, PseudoCostBranchNode
from simple_mip_solver_amd.generators import random_dense_milp_arrays
from tests.support.propagation_reference import mixed

pytestmark = pytest.mark.gpu
CASES = [(n, m, seed) for n, m in ((12, 6), (20, 10), (40, 20)) for seed in range(3)] + [('mixed', seed) for seed in range(2)]
STATS = ['rounds', 'base_rows', 'found', 'selected', 'kept', 'bound_before', 'bound_after', 'lp_pivots', 'kernel_us']


def arrays(case):
    if case[0] == 'mixed':
        return mixed(20, 10, 5, case[1])
    return random_dense_milp_arrays(case[0], case[1], seed=case[2])


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
    assert bb.root_cut_stats is None and bb.root_cuts is None
    return bb.status, float(bb.objective_value), bb.evaluated_nodes


@functools.lru_cache(maxsize=None)
def with_cuts(case):
    return search(case, root_cuts=True)


def close(a, b):
    """tests/test_engine_vs_highs_gpu.py's comparison of two optima: 1e-6 relative."""
    return abs(a - b) <= 1e-6 * max(1.0, abs(b))


def assert_optimal(bb, case):
    A, b, c, l, u, ints = arrays(case)
    assert bb.status == 'optimal' == plain(case)[0]
    print(case, bb.objective_value, plain(case)[1], highs_optimum(case), bb.evaluated_nodes, plain(case)[2], bb.root_cut_stats)
    assert close(bb.objective_value, plain(case)[1]) and close(bb.objective_value, highs_optimum(case))
    x = np.asarray(bb.solution, dtype=np.float64)
    assert x.shape == (len(c),) and close(float(c @ x), bb.objective_value)
    assert np.all(A @ x >= b - 1e-6) and np.all(x >= l - 1e-9) and np.all(x <= u + 1e-9)
    assert np.all(np.abs(x - np.round(x)) <= 1e-4)
    assert bb.model.A.shape == A.shape   # (the model is the one given: the cut rows live in the engine's problem)


@pytest.mark.parametrize('case', CASES, ids=str)
def test_search_with_root_cuts_finds_the_same_optimum(case):
    bb = with_cuts(case)
    assert_optimal(bb, case)
    st = bb.root_cut_stats
    assert list(st) == STATS
    assert st['kept'] == len(bb.root_cuts) <= 64 and st['selected'] >= st['kept'] and st['found'] >= st['selected']
    assert st['rounds'] >= 1 and st['base_rows'] >= st['rounds'] * arrays(case)[0].shape[0]
    assert st['bound_after'] >= st['bound_before'] - 1e-9 * abs(st['bound_before'])
    assert st['lp_pivots'] > 0 and st['kernel_us'] > 0
    for pi, pi0 in bb.root_cuts:
        assert pi.shape == (arrays(case)[0].shape[1],) and np.isfinite(pi0)
        x = np.asarray(bb.solution, dtype=np.float64)
        assert float(pi @ x) >= pi0 - 1e-6 * (abs(pi0) + float(np.abs(pi) @ np.abs(x)))   # (the optimum is not cut off)


def test_some_instance_keeps_cuts_and_gains_bound():
    kept = [with_cuts(case).root_cut_stats['kept'] for case in CASES]
    gain = [with_cuts(case).root_cut_stats['bound_after'] - with_cuts(case).root_cut_stats['bound_before'] for case in CASES]
    print(kept, gain)
    assert sum(kept) >= 1 and max(gain) > 1e-6


@pytest.mark.parametrize('case', [c for c in CASES if c[0] in (12, 20)], ids=str)
def test_the_kept_cuts_are_valid_by_highs(case):
    A, b, c, l, u, ints = arrays(case)
    for pi, pi0 in with_cuts(case).root_cuts[:12]:
        h = milp(pi, constraints=LinearConstraint(A, lb=b, ub=np.inf), bounds=Bounds(l, u), integrality=np.ones(len(c)),
                 options={'mip_rel_gap': 0.0})
        assert h.status == 0
        assert float(h.fun) >= pi0 - 1e-6 * (abs(pi0) + float(np.abs(pi) @ np.maximum(np.abs(l), np.abs(u)))), (h.fun, pi0)


@pytest.mark.parametrize('case', [(20, 10, 0), (40, 20, 1), ('mixed', 0)], ids=str)
def test_root_cuts_beside_the_other_options(case):
    bb = search(case, root_cuts=True, primal_heuristic=True, objective_step=True, reduced_cost=True, propagate=True)
    assert_optimal(bb, case)
    assert bb.heuristic_stats is not None and bb.propagation_stats['nodes'] > 0 and bb.root_cut_stats['rounds'] >= 1
    bb = search(case, Node=PseudoCostBranchDepthFirstSearchNode, root_cuts=3, root_cut_rows=8, primal_heuristic=True)
    assert_optimal(bb, case)
    assert bb.root_cut_stats['rounds'] <= 3 and len(bb.root_cuts) <= 8


def test_the_option_off_changes_nothing():
    case = (20, 10, 1)
    bb = search(case, root_cuts=None)
    assert bb.root_cut_stats is None and bb.root_cuts is None
    assert (bb.status, float(bb.objective_value), bb.evaluated_nodes) == plain(case)


def test_refused_combinations():
    A, b, c, l, u, ints = arrays((12, 6, 0))
    mdl = MILPInstance(A=A, b=b, c=c, l=l, u=u, sense=['Min', '>='], integerIndices=ints, numVars=len(c))

    def make(**kw):
        kw.setdefault('gomory_cuts', False)
        return BranchAndBound(mdl, PseudoCostBranchNode, pseudo_costs={}, **kw)

    with pytest.raises(AssertionError, match='root_cuts is None, True or a positive number of rounds'):
        make(frontier_batch=64, root_cuts=0)
    with pytest.raises(AssertionError, match='root_cuts is None, True or a positive number of rounds'):
        make(frontier_batch=64, root_cuts=2.5)
    with pytest.raises(AssertionError, match='root_cut_rows is None or a positive number of rows'):
        make(frontier_batch=64, root_cuts=True, root_cut_rows=0)
    with pytest.raises(AssertionError, match='root_cut_rows needs root_cuts'):
        make(frontier_batch=64, root_cut_rows=8)
    with pytest.raises(AssertionError, match='root_cuts needs frontier_batch'):
        make(root_cuts=True)
    with pytest.raises(AssertionError, match='root_cuts needs gomory_cuts=False'):
        make(frontier_batch=64, root_cuts=True, gomory_cuts=True)
    with pytest.raises(AssertionError, match='root_cuts cannot be combined with comm'):
        make(frontier_batch=64, root_cuts=True, comm=object())
    with pytest.raises(AssertionError, match='root_cuts cannot be combined with dual_function'):
        make(frontier_batch=64, root_cuts=True, dual_function=True)
    with pytest.raises(AssertionError, match='root_cuts cannot be combined with tree_record'):
        make(frontier_batch=64, root_cuts=True, tree_record=True)
