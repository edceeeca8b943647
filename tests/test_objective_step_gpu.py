"""The objective-step cutoff on the GPU (include/mipx_objstep.h): searches with the step against the search without
it and scipy's milp (HiGHS), beside every option it works with; the node counts with the primal heuristic; a node whose
LP value is exactly one step below the incumbent; other steps than 1; the engine's refusals."""
import functools

import numpy as np
import pytest
from scipy.optimize import Bounds, LinearConstraint, milp

from simple_mip_solver_amd import (BranchAndBound, MILPInstance, PseudoCostBranchDepthFirstSearchNode,
                                   PseudoCostBranchNode, _ffi)
from simple_mip_solver_amd.generators import random_dense_milp_arrays
from tests.support import propagation_reference as prop_ref
from tests.support.heuristic_reference import certify

pytestmark = pytest.mark.gpu
INF = float('inf')
INSTANCES = [('packing', seed) for seed in range(4)] + [('mixed', seed) for seed in range(4)]


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def arrays(family, seed):
    return random_dense_milp_arrays(40, 20, seed=seed) if family == 'packing' else prop_ref.mixed(20, 10, 5, seed)


def highs(A, b, c, l, u):
    h = milp(c, constraints=LinearConstraint(A, lb=b, ub=np.inf), bounds=Bounds(l, u), integrality=np.ones(len(c)),
             options={'mip_rel_gap': 0.0})
    assert h.status == 0
    return float(h.fun)


@functools.lru_cache(maxsize=None)
def highs_optimum(family, seed):
    A, b, c, l, u, ints = arrays(family, seed)
    return highs(A, b, c, l, u)


def search(family, seed, Node=PseudoCostBranchNode, frontier_batch=64, scale=1.0, **kw):
    A, b, c, l, u, ints = arrays(family, seed)
    mdl = MILPInstance(A=A, b=b, c=scale * c, l=l, u=u, sense=['Min', '>='], integerIndices=ints, numVars=len(c))
    bb = BranchAndBound(mdl, Node, pseudo_costs={}, gomory_cuts=False, mip_gap=0.0, frontier_batch=frontier_batch, **kw)
    bb.solve()
    return bb


@functools.lru_cache(maxsize=None)
def plain(family, seed):
    bb = search(family, seed)
    assert bb.objective_step_stats is None
    return bb.status, float(bb.objective_value), bb.evaluated_nodes


def close(a, b):
    """tests/test_engine_vs_highs_gpu.py's comparison of two optima: 1e-6 relative."""
    return abs(a - b) <= 1e-6 * max(1.0, abs(b))


def certified(bb):
    rs = bb.root_node.lp._engine_form()
    l, u = bb.root_node.lp._bounds()
    certify(rs.A, rs.b, rs.c, l, u, sorted(bb.model.integerIndices), np.asarray(bb.solution), bb.objective_value, tol=1e-6,
            int_tol=1e-4, obj_tol=1e-6)
    return True


def assert_optimal(bb, family, seed, what=''):
    status, value, nodes = plain(family, seed)
    native = bb._native.stats()
    print(what, family, seed, bb.status, bb.objective_value, value, highs_optimum(family, seed), 'dual', native['dual_bound'],
          'nodes', bb.evaluated_nodes, 'plain', nodes, bb.objective_step_stats)
    assert status == 'optimal' and bb.status == status, (what, seed, bb.status)
    assert close(bb.objective_value, value) and close(bb.objective_value, highs_optimum(family, seed)), \
        (what, seed, bb.objective_value, value, highs_optimum(family, seed))
    assert native['dual_bound'] == native['primal_bound'] == bb.objective_value   # (mip_gap 0: the gap is closed, not nearly)
    assert certified(bb)
    st = bb.objective_step_stats
    assert list(st) == list(_ffi.OBJSTEP_STATS_KEYS) and len(st) == 8 and not any(st[k] for k in _ffi.OBJSTEP_STATS_KEYS[3:])
    assert st['launches'] <= native['steps']
    assert bb._objective_step == 1.0   # (True became the gcd of the costs)


CONFIGS = [('alone', PseudoCostBranchNode, dict()),
           ('primal heuristic', PseudoCostBranchNode, dict(primal_heuristic=True)),
           ('local search', PseudoCostBranchNode, dict(primal_heuristic=True, local_search=True)),
           ('host spill, small pool', PseudoCostBranchNode, dict(host_spill=1 << 24, frontier_batch=16, pool_capacity=600)),
           ('no anchor', PseudoCostBranchNode, dict(anchor=False)),
           ('plunge of 8', PseudoCostBranchNode, dict(dive=8)),
           ('depth first', PseudoCostBranchDepthFirstSearchNode, dict()),
           ('propagation', PseudoCostBranchNode, dict(propagate=True)),
           ('reduced cost', PseudoCostBranchNode, dict(reduced_cost=True))]


@pytest.mark.parametrize('family,seed', INSTANCES)
@pytest.mark.parametrize('what,Node,kw', CONFIGS, ids=[c[0] for c in CONFIGS])
def test_search_with_the_step_finds_the_same_optimum(what, Node, kw, family, seed):
    bb = search(family, seed, Node, **dict(dict(objective_step=True), **kw))
    assert_optimal(bb, family, seed, what)
    if 'host_spill' in kw:
        assert bb.spill_stats is not None
    if 'primal_heuristic' in kw:
        assert bb.heuristic_stats['incumbents'] >= 1
    if 'local_search' in kw:
        assert bb.local_search_stats['points'] > 0
    if 'propagate' in kw:
        assert bb.propagation_stats['nodes'] > 0
    if 'reduced_cost' in kw:
        assert bb.reduced_cost_stats is not None


def test_fewer_nodes_with_the_heuristic_and_the_step():
    """An incumbent from step one and the step: summed over the four 40 x 20 seeds at frontier_batch 64 the search
    evaluates fewer nodes than with the heuristic alone, and the step closes nodes on at least one seed."""
    alone = [search('packing', seed, primal_heuristic=True) for seed in range(4)]
    both = [search('packing', seed, primal_heuristic=True, objective_step=True) for seed in range(4)]
    for seed in range(4):
        assert_optimal(both[seed], 'packing', seed, 'nodes')
        assert alone[seed].status == 'optimal' and alone[seed].objective_step_stats is None
    print('heuristic alone', [bb.evaluated_nodes for bb in alone], 'with the step', [bb.evaluated_nodes for bb in both],
          [bb.objective_step_stats for bb in both])
    assert sum(bb.evaluated_nodes for bb in both) < sum(bb.evaluated_nodes for bb in alone)
    assert any(bb.objective_step_stats['closed_at_pop'] + bb.objective_step_stats['left_unbranched'] > 0 for bb in both)


def test_a_node_exactly_one_step_below_the_incumbent_goes_on(gpu_ctx):
    """min -x0 - x1 + x2 with x0 + x1 <= 2, 2 x0 <= 3, 2 x1 <= 3: the root LP's optimal face is the segment from
    (1.5, 0.5, 0) to (0.5, 1.5, 0), value -2, both ends fractional, and (1, 1, 0) in its middle is the optimum.  With
    the incumbent (1, 0, 0) of value -1 and step 1 the root's value is exactly U - step: it branches, its children,
    which inherit -2, are popped, and the search ends on -2."""
    A = np.array([[-1.0, -1.0, 0.0], [-2.0, 0.0, 0.0], [0.0, -2.0, 0.0]]); b = np.array([-2.0, -3.0, -3.0])
    c = np.array([-1.0, -1.0, 1.0]); l = np.zeros(3); u = np.full(3, 3.0)
    assert highs(A, b, c, l, u) == -2.0 and np.all(A @ np.array([1.0, 0.0, 0.0]) >= b)
    p = _ffi.Problem(gpu_ctx, A, b, c)
    for step in (None, 1.0):
        t = _ffi.Tree(p, [0, 1, 2], l, u, branch_rule='most fractional', max_batch=1, pool_capacity=1 << 10)
        t.set_primal_bound(-1.0)
        if step:
            t.set_objective_step(step)
        t.set_trace(True)
        s = t.solve(mip_gap=0.0, frontier_batch=1)
        tr, st = t.trace(), t.objective_step_stats()
        print(step, s['status'], s['primal_bound'], s['dual_bound'], s['evaluated_nodes'], tr['objective'], tr['branch_var'], st)
        assert _ffi.TREE_STATUS[s['status']] == 'optimal' and s['primal_bound'] == -2.0 and s['dual_bound'] == -2.0
        assert abs(tr['objective'][0] + 2.0) <= 1e-9 and tr['branch_var'][0] >= 0   # (the root: exactly U - step, and it branched)
        assert s['evaluated_nodes'] >= 2
        assert np.allclose(t.solution(), [1.0, 1.0, 0.0], atol=1e-6)
        if not step:
            assert not any(st.values())
        t.close()
    p.close()


@pytest.mark.parametrize('seed', [0, 2])
def test_a_step_of_three_and_a_step_of_a_half(seed, gpu_ctx):
    """3 c: True finds the step 3.  c / 2: the step 0.5 has to be given, here through the C entry."""
    opt = highs_optimum('packing', seed)
    bb = search('packing', seed, scale=3.0, primal_heuristic=True, objective_step=True)
    assert bb._objective_step == 3.0 and bb.status == 'optimal' and close(bb.objective_value, 3.0 * opt) and certified(bb)
    st3 = bb.objective_step_stats
    one = search('packing', seed, scale=3.0, primal_heuristic=True, objective_step=1.0)   # (a divisor of the step is a step)
    print(seed, 'nodes: step 3', bb.evaluated_nodes, st3, 'step 1', one.evaluated_nodes, one.objective_step_stats)
    assert one.status == 'optimal' and close(one.objective_value, 3.0 * opt)
    assert st3['closed_at_pop'] + st3['left_unbranched'] > 0
    with pytest.raises(ValueError, match='pass the step'):
        search('packing', seed, scale=0.5, objective_step=True)
    A, b, c, l, u, ints = arrays('packing', seed)
    p = _ffi.Problem(gpu_ctx, A, b, 0.5 * c)
    t = _ffi.Tree(p, ints, l, u, branch_rule='pseudo cost', max_batch=64, pool_capacity=1 << 16)
    t.set_anchor_mode(True)
    t.set_dive(True)
    t.set_heuristic(True)
    t.set_objective_step(0.5)
    s = t.solve(mip_gap=0.0, frontier_batch=64)
    st = t.objective_step_stats()
    print(seed, 'step 0.5', s['evaluated_nodes'], st)
    assert _ffi.TREE_STATUS[s['status']] == 'optimal' and close(s['primal_bound'], 0.5 * opt) and s['dual_bound'] == s['primal_bound']
    certify(A, b, 0.5 * c, l, u, ints, t.solution(), s['primal_bound'], tol=1e-6, int_tol=1e-4, obj_tol=1e-6)
    assert st['closed_at_pop'] + st['left_unbranched'] > 0 and st['launches'] > 0
    t.close()
    p.close()


def test_engine_refusals(gpu_ctx):
    A, b, c, l, u, ints = random_dense_milp_arrays(20, 10, seed=3)
    p = _ffi.Problem(gpu_ctx, A, b, c)

    def tree(**kw):
        return _ffi.Tree(p, ints, l, u, max_batch=4, pool_capacity=1 << 12, **kw)

    t = tree(cut_params={})
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*mipx_tree_set_objective_step: not with cut rounds'):
        t.set_objective_step(1.0)
    t.close()
    t = tree()
    for bad in (0.0, -1.0, INF, float('nan')):
        with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*the step is positive and finite'):
            t.set_objective_step(bad)
    assert not any(t.objective_step_stats().values())
    t.set_objective_step(1.0)
    comm = _ffi.Comm(gpu_ctx, 0, 1, allgather=lambda buf: [buf], send=lambda peer, d: None, recv=lambda peer, k: b'')
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*mipx_tree_set_comm: not with the objective step'):
        t.set_comm(comm, 3)
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*mipx_tree_set_tree_record: not with the objective step'):
        t.set_tree_record(True)
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*mipx_tree_set_dual_record: not with the objective step'):
        t.set_dual_record(1 << 20, 10, np.arange(10, dtype=np.int32), np.ones(10))
    t.set_objective_step(2.0)   # (set again before the first step: the last one holds)
    t.solve(frontier_batch=4, max_steps=1)
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*before the first step'):
        t.set_objective_step(1.0)
    t.close()
    t = tree()
    t.solve(frontier_batch=4, max_steps=1)   # (a tree that has stepped without it)
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*before the first step'):
        t.set_objective_step(1.0)
    t.close()
    t = tree()
    t.set_comm(comm, 3)
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*mipx_tree_set_objective_step: not with a communicator'):
        t.set_objective_step(1.0)
    t.set_comm(None)
    t.close()
    t = tree()
    t.set_tree_record(True)
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*mipx_tree_set_objective_step: not with the tree record'):
        t.set_objective_step(1.0)
    t.close()
    t = tree()
    t.set_dual_record(1 << 20, 10, np.arange(10, dtype=np.int32), np.ones(10))
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*mipx_tree_set_objective_step: not with the dual function'):
        t.set_objective_step(1.0)
    t.close()
    # a tree seeded from a recorded one keeps the record on, and is refused with it
    src = tree()
    src.set_tree_record(True)
    src.solve(mip_gap=0.0, frontier_batch=4, max_steps=3)
    p2 = _ffi.Problem(gpu_ctx, A, b - 1.0, c)
    t = _ffi.Tree.restart(src, p2)
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*mipx_tree_set_objective_step: not with the tree record'):
        t.set_objective_step(1.0)
    t.close()
    src.close()
    p2.close()
    comm.close()
    p.close()


@pytest.mark.parametrize('rule,batch', [('pseudo cost', 1), ('most fractional', 64)])
def test_a_tree_that_never_sets_the_option_is_unchanged(rule, batch, gpu_ctx):
    """Two trees on one instance, neither option set, the trace on: the same trace, node for node, and none of the
    counters of either option moves.  (The two configurations whose node order does not depend on when the host
    finishes a step: one node per step, and batches without a pseudo-cost table.)"""
    A, b, c, l, u, ints = random_dense_milp_arrays(40, 20, seed=0)

    def run():
        p = _ffi.Problem(gpu_ctx, A, b, c)   # (a problem of its own: the anchor a search sets stays on its problem)
        t = _ffi.Tree(p, ints, l, u, branch_rule=rule, max_batch=batch, pool_capacity=1 << 16)
        if batch > 1:
            t.set_anchor_mode(True)
            t.set_dive(True)
        t.set_trace(True)
        st = t.solve(mip_gap=0.0, frontier_batch=batch, node_limit=3000)
        out = st, t.trace(), t.objective_step_stats(), t.local_search_stats()
        t.close()
        p.close()
        return out

    st1, tr1, o1, l1 = run()
    st2, tr2, o2, l2 = run()
    assert st1['status'] == st2['status'] and st1['primal_bound'] == st2['primal_bound'] and st1['evaluated_nodes'] > 100
    for key in ('evaluated_nodes', 'lp_solved', 'pivots', 'created_nodes', 'steps', 'dives'):
        assert st1[key] == st2[key], key
    for key in ('node_id', 'status', 'branch_var'):
        assert np.array_equal(tr1[key], tr2[key]), key
    assert np.array_equal(bits(tr1['objective']), bits(tr2['objective']))
    assert list(o1) == list(_ffi.OBJSTEP_STATS_KEYS) and len(o1) == 8 and not any(o1.values()) and not any(o2.values())
    assert not any(l1.values()) and not any(l2.values())
