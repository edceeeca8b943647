"""Clique cuts in the native search (BranchAndBound(root_cuts=..., clique_cuts=True), include/mipx_clique.h) on the
conflict packing family: the search with the option ends at scipy's milp (HiGHS) optimum, every cut it keeps is valid
by HiGHS, the counters of the three cut kinds add up, the search without the option is as before, what the
constructor refuses, and the two stand-alone entries of utils/clique_cuts.py on a search and on a model."""
import functools

import numpy as np
import pytest
from scipy.optimize import Bounds, LinearConstraint, milp

from simple_mip_solver_amd import BranchAndBound, MILPInstance, PseudoCostBranchNode
from simple_mip_solver_amd.generators import conflict_packing_milp_arrays, random_dense_milp_arrays
from simple_mip_solver_amd.utils import clique_cuts
from tests.support import clique_reference as ref

pytestmark = pytest.mark.gpu
SHAPE = (24, 70, 4, 8)
EDGES = {0: 113, 1: 112}
CLIQUE_STATS = ['rounds', 'seeds', 'found', 'selected', 'kept', 'edges', 'rows_skipped', 'kernel_us']


def model_of(arrays):
    A, b, c, l, u, ints = arrays
    return MILPInstance(A=A.copy(), b=b.copy(), c=c.copy(), l=l.copy(), u=u.copy(), sense=['Min', '>='],
                        integerIndices=list(ints), numVars=len(c))


@functools.lru_cache(maxsize=None)
def highs_optimum(seed):
    A, b, c, l, u, ints = conflict_packing_milp_arrays(*SHAPE, seed=seed)
    h = milp(c, constraints=LinearConstraint(A, lb=b, ub=np.inf), bounds=Bounds(l, u), integrality=np.ones(len(c)),
             options={'mip_rel_gap': 0.0})
    assert h.status == 0
    return float(h.fun)


@functools.lru_cache(maxsize=None)
def search(seed, clique):
    kw = dict(clique_cuts=True) if clique else {}
    bb = BranchAndBound(model_of(conflict_packing_milp_arrays(*SHAPE, seed=seed)), Node=PseudoCostBranchNode, pseudo_costs={},
                        gomory_cuts=False, frontier_batch=64, root_cuts=True, cover_cuts=True, **kw)
    bb.solve()
    return bb


def close(a, b):
    return abs(a - b) <= 1e-6 * max(1.0, abs(b))


@pytest.mark.parametrize('seed', [0, 1])
def test_the_search_with_clique_cuts_proves_the_highs_optimum(seed):
    A, b, c, l, u, ints = conflict_packing_milp_arrays(*SHAPE, seed=seed)
    bb, off = search(seed, True), search(seed, False)
    st, cs, qs = bb.root_cut_stats, bb.cover_cut_stats, bb.clique_cut_stats
    print(seed, 'with cliques: root bound', st['bound_before'], '->', st['bound_after'], 'nodes', bb.evaluated_nodes, qs)
    print(seed, 'without:      root bound', off.root_cut_stats['bound_before'], '->', off.root_cut_stats['bound_after'],
          'nodes', off.evaluated_nodes, 'optimum', highs_optimum(seed))
    assert bb.status == 'optimal' and close(bb.objective_value, highs_optimum(seed))
    x = np.asarray(bb.solution, dtype=np.float64)
    assert close(float(c @ x), bb.objective_value) and np.all(A @ x >= b - 1e-6) and np.all(np.abs(x - np.round(x)) <= 1e-4)
    assert list(qs) == CLIQUE_STATS
    assert qs['edges'] == EDGES[seed] and qs['rows_skipped'] == 0 and qs['kernel_us'] > 0
    assert qs['rounds'] == st['rounds'] == cs['rounds'] >= 1 and qs['seeds'] == 48 * qs['rounds']
    assert 1 <= qs['kept'] <= qs['selected'] <= qs['found']
    assert st['kept'] + cs['kept'] + qs['kept'] == len(bb.root_cuts)
    for pi, pi0 in bb.root_cuts:
        h = milp(pi, constraints=LinearConstraint(A, lb=b, ub=np.inf), bounds=Bounds(l, u), integrality=np.ones(len(c)),
                 options={'mip_rel_gap': 0.0})
        assert h.status == 0
        assert float(h.fun) >= pi0 - 1e-6 * (abs(pi0) + float(np.abs(pi) @ np.maximum(np.abs(l), np.abs(u)))), (h.fun, pi0)
    # the same search without the option: no counters, the same optimum
    assert off.clique_cut_stats is None and off.status == 'optimal' and close(off.objective_value, highs_optimum(seed))
    assert off.root_cut_stats['kept'] + off.cover_cut_stats['kept'] == len(off.root_cuts)


def test_general_integers_give_no_clique_and_the_same_search():
    arrays = random_dense_milp_arrays(20, 10, seed=1)

    def run(**kw):
        bb = BranchAndBound(model_of(arrays), Node=PseudoCostBranchNode, pseudo_costs={}, gomory_cuts=False, mip_gap=0.0,
                            frontier_batch=64, root_cuts=True, **kw)
        bb.solve()
        return bb
    mir, bb = run(), run(clique_cuts=True)
    qs = bb.clique_cut_stats
    assert qs['found'] == qs['selected'] == qs['kept'] == qs['edges'] == 0 and qs['rounds'] == bb.root_cut_stats['rounds']
    assert (bb.status, float(bb.objective_value), bb.evaluated_nodes) == \
        (mir.status, float(mir.objective_value), mir.evaluated_nodes)
    assert len(bb.root_cuts) == len(mir.root_cuts) and all(
        np.array_equal(p, q) and p0 == q0 for (p, p0), (q, q0) in zip(bb.root_cuts, mir.root_cuts))
    assert mir.clique_cut_stats is None and bb.cover_cut_stats is None


def test_refused_combinations():
    mdl = model_of(conflict_packing_milp_arrays(16, 36, 3, 6, seed=0))

    def make(**kw):
        kw.setdefault('gomory_cuts', False)
        return BranchAndBound(mdl, PseudoCostBranchNode, pseudo_costs={}, **kw)

    with pytest.raises(AssertionError, match='clique_cuts needs root_cuts'):
        make(frontier_batch=64, clique_cuts=True)
    for bad in (False, 1, 3, 'yes'):
        with pytest.raises(AssertionError, match='clique_cuts is None or True'):
            make(frontier_batch=64, root_cuts=True, clique_cuts=bad)
    with pytest.raises(AssertionError, match='root_cuts needs frontier_batch'):
        make(root_cuts=True, clique_cuts=True)
    bb = make(frontier_batch=64, root_cuts=True, clique_cuts=True)
    assert bb._clique_cuts is True and bb._cover_cuts is False and bb.clique_cut_stats is None
    bb = make(frontier_batch=64, root_cuts=True, cover_cuts=True)
    assert bb._clique_cuts is False and bb.clique_cut_stats is None


def test_the_stand_alone_entries_on_a_search_and_on_a_model():
    arrays = conflict_packing_milp_arrays(16, 36, 3, 6, seed=1)
    A, b, c, l, u, ints = arrays
    exp_adj, _ = ref.graph(A, b, l, u, ints)
    X = np.full((2, 16), 0.5)
    X[1, ::3] = 0.25
    exp = ref.separate(X, l, u, ints, exp_adj)
    bb = BranchAndBound(model_of(arrays), PseudoCostBranchNode, pseudo_costs={}, gomory_cuts=False, frontier_batch=64)
    for target in (model_of(arrays), bb):
        adj = clique_cuts.conflict_graph(target)
        assert adj.dtype == np.uint32 and np.array_equal(adj, ref.pack(exp_adj))
        assert np.array_equal(clique_cuts.unpack_adjacency(adj, 16), exp_adj)
        for given in (None, adj):
            pi, pi0, eff, size, status = clique_cuts.separate_cliques(target, X, adj=given)
            assert pi.shape == (2, 32, 16) and np.array_equal(status, exp['status']) and np.array_equal(size, exp['size'])
            assert np.array_equal(pi, exp['pi']) and np.array_equal(pi0, exp['pi0'])
            assert np.array_equal(eff.view(np.int64), exp['efficacy'].view(np.int64))
        one = clique_cuts.separate_cliques(target, X[0], seeds=[4, 0], min_efficacy=-np.inf)
        assert one[0].shape == (1, 2, 16) and np.array_equal(one[3][0], exp['size'][0, [4, 0]])
    # a box of the caller's: with column 0 fixed at 0 its literals leave the graph
    u2 = u.copy()
    u2[0] = 0.0
    adj2 = clique_cuts.conflict_graph(bb, l=l, u=u2)
    assert np.array_equal(adj2, ref.pack(ref.graph(A, b, l, u2, ints)[0])) and not adj2[:2].any()
    with pytest.raises(AssertionError, match='one point of n columns'):
        clique_cuts.separate_cliques(bb, X[:, :5])
    with pytest.raises(AssertionError, match='list of literals'):
        clique_cuts.separate_cliques(bb, X, seeds=[0.5])
    with pytest.raises(AssertionError, match='one box of n columns'):
        clique_cuts.conflict_graph(bb, l=np.zeros(3), u=np.ones(3))
    with pytest.raises(AssertionError, match='BranchAndBound or a MILPInstance'):
        clique_cuts.conflict_graph(object())
    with pytest.raises(AssertionError, match='BranchAndBound or a MILPInstance'):
        clique_cuts.separate_cliques(object(), X)
