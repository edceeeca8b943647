"""BranchAndBound(lp_batch=B): user node classes and queues on the Python loop, with the first LP of B
popped nodes solved in one engine launch per row set.  Runs on the CPU oracle (`-m "not gpu"`) and on
the HIP engine (`-m gpu`) through the `engine` fixture."""
import os
from math import ceil, floor

import numpy as np
import pytest

from simple_mip_solver_amd import BaseNode, BranchAndBound, MILPInstance, PseudoCostBranchNode
from simple_mip_solver_amd.generators import random_dense_milp_arrays
from simple_mip_solver_amd.lp import CyLPArray
from tests.support.example_models import model

HERE = os.path.dirname(os.path.abspath(__file__))
MPS = ['constraints_high_variables_high_density_high_max_obj_coeff_high_max_cons_coeff_high_tightness_low.mps',
       'constraints_high_variables_high_density_low_max_obj_coeff_high_max_cons_coeff_high_tightness_low.mps']
INSTANCES = ['small_branch', 'random_10x5'] + MPS


def instance(name):
    if name.endswith('.mps'):
        return MILPInstance(file_name=os.path.join(HERE, 'golden', 'example_models', name))
    if name.startswith('random'):
        A, b, c, l, u, ints = random_dense_milp_arrays(10, 5, seed=3)
        return MILPInstance(A=A, b=b, c=c, l=l, u=u, sense=['Min', '>='], integerIndices=ints, numVars=10)
    return model(name)


class LeastFractionalNode(BaseNode):
    """A user's node: branches on the least fractional variable, prefers deeper nodes on ties, and
    records the order it is bounded in."""
    log = None

    def bound(self, **kwargs):
        if LeastFractionalNode.log is not None:
            LeastFractionalNode.log.append(self.idx)
        return super().bound(**kwargs)

    def branch(self, **kwargs):
        frac = self._fractional_indices()
        dist = [min(self.solution[i] - floor(self.solution[i]), ceil(self.solution[i]) - self.solution[i])
                for i in frac]
        return self._base_branch(frac[int(np.argmin(dist))], **kwargs)

    def __lt__(self, other):
        return (self.dual_bound, -self.depth) < (other.dual_bound, -other.depth)


class TighteningNode(LeastFractionalNode):
    """Changes its LP's bounds before bounding: a result solved ahead must not be taken."""

    def bound(self, **kwargs):
        # strictly below the bound the node inherited (unless x0 was branched on), above any x0 feasible here
        self.lp.variablesUpper[0] = min(self.lp.variablesUpper[0], 99 + 0.5 ** (self.depth + 1))
        return super().bound(**kwargs)


class SharingNode(LeastFractionalNode):
    """Returns one slack cut per node (sum x >= -1), which BranchAndBound shares with every node
    still waiting; records which shared cuts each node holds when it is bounded."""
    pools = None

    def bound(self, **kwargs):
        SharingNode.pools[self.idx] = set(self.cut_pool)
        rtn = super().bound(**kwargs)
        rtn['cuts'] = {f'cut_shared_{self.idx}': (CyLPArray(np.ones(self.lp.nVariables)), -1.0)}
        return rtn


class Lifo:
    def __init__(self):
        self.items = []

    def put(self, node):
        self.items.append(node)

    def get(self):
        return self.items.pop()

    def empty(self):
        return not self.items


def counting(engine, monkeypatch):
    box = dict(calls=0, lps=0)
    inner = engine.solve

    def solve(A, b, c, l, u, vstat, max_iter, cache_key):
        box['calls'] += 1
        box['lps'] += len(l)
        return inner(A, b, c, l, u, vstat, max_iter, cache_key)
    monkeypatch.setattr(engine, 'solve', solve)
    return box


def run(name, Node=LeastFractionalNode, **kw):
    LeastFractionalNode.log = []
    kw.setdefault('gomory_cuts', False)
    bb = BranchAndBound(instance(name), Node=Node, **kw)
    bb.solve()
    order, LeastFractionalNode.log = LeastFractionalNode.log, None
    return bb, order


def tree_record(bb):
    return sorted((v.attr['node'].idx, v.attr['node'].dual_bound, v.attr['node'].objective_value,
                   v.attr['node'].lp_feasible, v.attr['node'].mip_feasible) for v in bb.tree.nodes.values())


def assert_same_result(a, b, exact=True):
    assert a.status == b.status
    if exact:
        assert a.objective_value == b.objective_value
        assert (a.solution is None) == (b.solution is None)
        if a.solution is not None:
            assert np.array_equal(a.solution, b.solution)
    else:
        assert a.objective_value == pytest.approx(b.objective_value, rel=1e-9, abs=1e-9)


@pytest.mark.parametrize('name', INSTANCES)
def test_lp_batch_1_equals_per_node(engine, name):
    ref, ref_order = run(name)
    bb, order = run(name, lp_batch=1)
    assert order == ref_order and bb.evaluated_nodes == ref.evaluated_nodes
    assert tree_record(bb) == tree_record(ref)
    assert {k: v for k, v in bb._kwargs.items()} == {k: v for k, v in ref._kwargs.items()}
    assert_same_result(bb, ref)
    assert bb.lp_batch_stats['consumed'] == bb.evaluated_nodes


@pytest.mark.parametrize('B', [4, 64])
@pytest.mark.parametrize('name', INSTANCES)
def test_lp_batch_fewer_launches_same_optimum(engine, monkeypatch, name, B):
    ref, _ = run(name)
    box = counting(engine, monkeypatch)
    bb, order = run(name, lp_batch=B)
    assert_same_result(bb, ref, exact=False)
    assert 'lp_batch' not in bb._kwargs
    assert box['calls'] < box['lps'], box
    st = bb.lp_batch_stats
    assert st['launches'] == box['calls'] and st['prefetched'] == box['lps']
    assert st['consumed'] + st['wasted'] == st['prefetched'] and st['consumed'] == len(order)


def test_lp_batch_custom_queue(engine, monkeypatch):
    ref, ref_order = run('random_10x5', node_queue=Lifo())
    one, one_order = run('random_10x5', node_queue=Lifo(), lp_batch=1)
    assert one_order == ref_order
    assert_same_result(one, ref)
    box = counting(engine, monkeypatch)
    bb, _ = run('random_10x5', node_queue=Lifo(), lp_batch=8)
    assert_same_result(bb, ref, exact=False)
    assert box['calls'] < box['lps']


@pytest.mark.parametrize('name', MPS)
def test_changed_lp_is_solved_again(engine, name):
    ref, ref_order = run(name, Node=TighteningNode)
    bb, order = run(name, Node=TighteningNode, lp_batch=1)
    assert order == ref_order and tree_record(bb) == tree_record(ref)
    assert_same_result(bb, ref)
    assert bb.lp_batch_stats['wasted'] > 0
    b4, _ = run(name, Node=TighteningNode, lp_batch=4)
    assert_same_result(b4, ref, exact=False)
    assert b4.lp_batch_stats['wasted'] > 0


@pytest.mark.parametrize('name', ['small_branch', 'random_10x5'])
def test_pseudo_cost_node(engine, name):
    ref = BranchAndBound(instance(name), Node=PseudoCostBranchNode, pseudo_costs={})
    ref.solve()
    one = BranchAndBound(instance(name), Node=PseudoCostBranchNode, pseudo_costs={}, lp_batch=1)
    one.solve()
    assert tree_record(one) == tree_record(ref) and one._kwargs == ref._kwargs
    assert_same_result(one, ref)
    bb = BranchAndBound(instance(name), Node=PseudoCostBranchNode, pseudo_costs={}, lp_batch=16)
    bb.solve()
    assert_same_result(bb, ref, exact=False)


@pytest.mark.parametrize('name', ['small_branch', MPS[1]])
def test_gomory_cuts(engine, name):
    ref, _ = run(name, gomory_cuts=True)
    one, _ = run(name, gomory_cuts=True, lp_batch=1)
    assert tree_record(one) == tree_record(ref) and one._kwargs == ref._kwargs
    bb, _ = run(name, gomory_cuts=True, lp_batch=8)
    assert_same_result(bb, ref, exact=False)


def test_shared_cuts_reach_popped_nodes(engine):
    """A node that was waiting (in the queue, or taken off it by this step and not yet bounded) when
    another node returned a cut holds that cut when it is bounded."""
    for B in (None, 1, 8):
        SharingNode.pools = {}
        bb, order = run('random_10x5', Node=SharingNode, lp_batch=B)
        parent = {v.attr['node'].idx: v.attr['node'].lineage[-2] for v in bb.tree.nodes.values()
                  if v.attr['node'].lineage and len(v.attr['node'].lineage) > 1}
        at = {idx: k for k, idx in enumerate(order)}
        assert len(order) > 8
        for idx in order:
            if idx not in parent:
                continue
            born = at[parent[idx]]
            want = {f'cut_shared_{w}' for w in order[born + 1:at[idx]]}
            assert SharingNode.pools[idx] == want, (B, idx)


def test_argument_checks():
    m = model('small_branch')
    with pytest.raises(AssertionError, match='lp_batch must be a positive integer'):
        BranchAndBound(m, lp_batch=0)
    with pytest.raises(AssertionError, match='lp_batch must be a positive integer'):
        BranchAndBound(m, lp_batch=-3)
    with pytest.raises(AssertionError, match='lp_batch must be a positive integer'):
        BranchAndBound(m, lp_batch=2.0)
    with pytest.raises(AssertionError, match='cannot be combined with frontier_batch'):
        BranchAndBound(m, lp_batch=4, frontier_batch=4)
    with pytest.raises(AssertionError, match='cannot be combined with comm'):
        BranchAndBound(m, lp_batch=4, comm=object())
    bb = BranchAndBound(m, Node=LeastFractionalNode, node_queue=Lifo(), lp_batch=4)
    assert bb.lp_batch == 4 and 'lp_batch' not in bb._kwargs
