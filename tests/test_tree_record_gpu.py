"""The tree record of the frontier engine (BranchAndBound(frontier_batch=B, tree_record=True),
include/mipx_treerec.h).  The comparator is always the Python loop (frontier_batch=None) or HiGHS, never the
engine's own record: node-for-node parity at frontier_batch=1, the bounds kernel against the pool rows of the
open nodes, the structure of a batched search, the batched re-solve under the LP certificate, the disjunctive
cut from a recorded tree, and the record next to the other options."""
import glob
import os

import numpy as np
import pytest
from scipy.optimize import linprog

from simple_mip_solver_amd import BaseNode, BranchAndBound, MILPInstance, PseudoCostBranchNode, _ffi
from simple_mip_solver_amd.generators import random_dense_milp_arrays
from simple_mip_solver_amd.utils.cut_generating_lp import CutGeneratingLP
from tests.support import lp_certificate as cert
from tests.support.example_models import model, std_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.abspath(__file__))
INF = float('inf')


def generator_model(n, m, seed):
    A, b, c, l, u, ints = random_dense_milp_arrays(n, m, seed=seed)
    return MILPInstance(A=A, b=b, c=c, l=l, u=u, sense=['Min', '>='], integerIndices=ints, numVars=n)


def close(a, b, rel=1e-9):
    return abs(a - b) <= rel * max(1.0, abs(a), abs(b))


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def value_function_models():
    folders = sorted(glob.glob(os.path.join(ROOT, 'golden', 'example_value_functions', 'instance_*')))
    assert len(folders) == 5
    return [(lambda f=os.path.join(folder, 'evaluation_0.mps'): MILPInstance(file_name=f)) for folder in folders]


PARITY_MODELS = [('small_branch', lambda: model('small_branch')), ('std small_branch', lambda: std_model('small_branch')),
                 ('h3p1', lambda: model('h3p1'))] + \
                [(f'value function {k}', f) for k, f in enumerate(value_function_models())] + \
                [(f'generator {n}x{m}', (lambda n=n, m=m: generator_model(n, m, 3))) for n, m in ((20, 10), (30, 15), (40, 20))]


def solved_pair(factory, Node, node_limit, **extra):
    kw = dict(gomory_cuts=False, node_limit=node_limit)
    if Node is PseudoCostBranchNode:
        kw['pseudo_costs'] = {}
    py = BranchAndBound(factory(), Node, **kw)
    py.solve()
    if Node is PseudoCostBranchNode:
        kw['pseudo_costs'] = {}
    bb = BranchAndBound(factory(), Node, frontier_batch=1, tree_record=True, **kw, **extra)
    bb.solve()
    return py, bb


def same_value(a, b, what):
    """None, +-inf or the same bits."""
    if a is None or b is None:
        assert a is None and b is None, what
    else:
        assert np.array_equal(bits([a]), bits([b])), (what, a, b)


def assert_same_tree(py, bb, what):
    pt, nt = py.tree, bb.tree
    assert sorted(pt.nodes) == sorted(nt.nodes), what
    ids = sorted(pt.nodes)
    mine = dict(zip(ids, nt._instances(ids)))   # (one bounds query for the whole tree)
    for i in ids:
        a, b, w = pt.nodes[i].attr['node'], mine[i], (what, i)
        assert isinstance(b, bb._Node) and b.idx == a.idx == i, w
        assert pt.get_parent(i) == nt.get_parent(i), w
        assert pt.get_left_child(i) == nt.get_left_child(i) and pt.get_right_child(i) == nt.get_right_child(i), w
        assert pt.get_children(i) == nt.get_children(i), w
        assert a.lineage == b.lineage and a.depth == b.depth and a.is_leaf == b.is_leaf, w
        assert a.lp_feasible is b.lp_feasible and a.mip_feasible is b.mip_feasible and a.unbounded is b.unbounded, \
            (w, a.lp_feasible, b.lp_feasible, a.mip_feasible, b.mip_feasible)
        assert a._b_idx == b._b_idx and a._b_dir == b._b_dir, w
        assert np.array_equal(bits(a.lp.variablesLower), bits(b.lp.variablesLower)), w
        assert np.array_equal(bits(a.lp.variablesUpper), bits(b.lp.variablesUpper)), w
        # exact mode runs the same kernels on the same LPs in the same order: bit for bit
        same_value(a._b_val, b._b_val, w + ('b_val',))
        same_value(a.dual_bound, b.dual_bound, w + ('dual_bound',))
        same_value(a.objective_value, b.objective_value, w + ('objective_value',))
    assert nt.get_node_instances(0) is bb.root_node and bb.root_node.idx in nt
    # get_leaves for every subtree root, depth and keep.  The Python tree's method scans every vertex per call,
    # so on a tree of thousands of nodes the expected sets are collected in one pass over the Python loop's
    # nodes by the method's own definition (is_leaf, lineage, lp_feasible of those nodes), and the method
    # itself is called for every root of a small tree and for a fixed sample of roots of a large one.
    depths, keeps = (None, 0, 1, 2, 3), ('all', 'feasible', 'not infeasible')
    kept = {'all': lambda n: True, 'feasible': lambda n: bool(n.lp_feasible),
            'not infeasible': lambda n: n.lp_feasible is not False}
    want = {(r, d): [] for r in ids for d in depths}
    for i in ids:
        n = pt.nodes[i].attr['node']
        want[i, 0].append(n)
        if len(n.lineage) > 1:
            want[n.lineage[-2], 1].append(n)
        if n.is_leaf:
            for r in n.lineage:
                want[r, None].append(n)
        for d in (2, 3):
            if n.is_leaf:
                for r in n.lineage[-d:]:
                    want[r, d].append(n)
            if len(n.lineage) >= d + 1:
                want[n.lineage[-(d + 1)], d].append(n)
    sample = set(ids) if len(ids) <= 200 else set(np.random.default_rng(1).choice(ids, 40, replace=False).tolist()) | {0, 1, 2}
    for r in ids:
        for d in depths:
            for keep in keeps:
                exp = sorted(n.idx for n in want[r, d] if kept[keep](n))
                assert exp == sorted(nt.get_leaf_ids(r, depth=d, keep=keep)), (what, r, d, keep)
                if r in sample:
                    assert exp == sorted(n.idx for n in pt.get_leaves(r, depth=d, keep=keep)), (what, r, d, keep)
                    assert exp == sorted(n.idx for n in nt.get_leaves(r, depth=d, keep=keep)), (what, r, d, keep)
            if want[r, d]:
                value = min(n.objective_value if n.objective_value is not None else n.dual_bound for n in want[r, d])
                same_value(value, nt.subtree_dual_bound(r, depth=d), (what, r, d, 'subtree_dual_bound'))
                if r in sample:
                    same_value(pt.subtree_dual_bound(r, depth=d), value, (what, r, d, 'python subtree_dual_bound'))
    dp, dn = pt.get_disjunction(0), nt.get_disjunction(0)
    assert sorted(dp) == sorted(dn), what
    for i in dp:
        assert np.array_equal(bits(dp[i][0]), bits(dn[i][0])) and np.array_equal(bits(dp[i][1]), bits(dn[i][1])), (what, i)


# ---- 1. node-for-node parity at frontier_batch = 1 --------------------------------------------------
@pytest.mark.parametrize('node_limit', [INF, 15])
@pytest.mark.parametrize('Node', [BaseNode, PseudoCostBranchNode])
@pytest.mark.parametrize('name,factory', PARITY_MODELS, ids=[n for n, _ in PARITY_MODELS])
def test_parity_with_the_python_loop(name, factory, Node, node_limit):
    py, bb = solved_pair(factory, Node, node_limit)
    assert bb.evaluated_nodes == py.evaluated_nodes and bb.status == py.status
    assert_same_tree(py, bb, (name, Node.__name__, node_limit))
    st = bb.tree_record_stats
    assert st['nodes'] == len(py.tree.nodes) and st['host_bytes'] >= 14 * st['nodes']


def test_known_id_sets_of_small_branch():
    """The sets tests/test_branch_and_bound.py pins on the Python tree, out of the native one, across a
    re-entrant solve."""
    bb = BranchAndBound(std_model('small_branch'), gomory_cuts=False, node_limit=1, frontier_batch=1, tree_record=True)
    bb.solve()
    assert len(bb.tree.get_leaves(0, keep='not infeasible')) == 2
    assert not bb.tree.get_leaves(0, keep='feasible')
    early = bb.tree.get_node_instances(1)
    assert early.lp_feasible is None and early.solution is None
    bb.node_limit = INF
    bb.solve()
    assert bb.tree.get_node_instances(1) is early and early.lp_feasible is True   # (brought up to date)
    assert sorted(bb.tree.nodes) == list(range(13))
    leaves = {n.idx for n in bb.tree.get_leaves(0)}
    for node_id in bb.tree.nodes:
        assert len(bb.tree.get_children(node_id)) == (0 if node_id in leaves else 2)
    assert {n.idx for n in bb.tree.get_leaves(0) if not n.lp_feasible} == {2, 6, 8, 10, 12}
    assert [n.idx for n in bb.tree.get_leaves(2, depth=0)] == [2]
    assert not bb.tree.get_leaves(2, depth=0, keep='feasible')
    assert {n.idx for n in bb.tree.get_leaves(0, depth=1)} == {1, 2}
    assert [n.idx for n in bb.tree.get_leaves(0, depth=1, keep='feasible')] == [1]
    assert {n.idx for n in bb.tree.get_leaves(1, depth=2)} == {5, 6, 7, 8}
    assert {n.idx for n in bb.tree.get_leaves(1, depth=2, keep='feasible')} == {5, 7}
    assert {n.idx for n in bb.tree.get_leaves(1, depth=3)} == {5, 6, 8, 9, 10}
    assert {n.idx for n in bb.tree.get_leaves(1, depth=3, keep='feasible')} == {5, 9}
    for n in bb.tree.get_leaves(1, depth=2):
        assert bb.tree.get_parent(bb.tree.get_parent(n.idx)) == 1
    d = bb.tree.get_disjunction(0)
    assert set(d) == {5, 11}
    assert all(d[5][0] == [0, 0, 0]) and all(d[5][1] == [0, 1, 1])
    assert all(d[11][0] == [1, 0, 0]) and all(d[11][1] == [1, 1, 0])
    with pytest.raises(AssertionError, match='subtree_root_id must belong to the tree'):
        bb.tree.get_leaves(20)
    with pytest.raises(AssertionError, match='depth is a nonnegative integer'):
        bb.tree.get_leaves(subtree_root_id=0, depth=1.5)
    with pytest.raises(AssertionError, match="keep is one of 'all', 'feasible', or 'not infeasible'"):
        bb.tree.get_leaves(subtree_root_id=0, keep=False)
    with pytest.raises(AssertionError, match='not in the tree'):
        bb.tree.get_node_instances([0, 20])


# ---- 2. the kernel against the pool rows of the open nodes ---------------------------------------------
@pytest.mark.parametrize('batch,dive,rule', [(1, 0, 'most fractional'), (64, 2, 'pseudo cost'), (256, 1, 'pseudo cost')])
def test_open_nodes_bounds_equal_their_pool_rows(batch, dive, rule, gpu_ctx):
    A, b, c, l, u, ints = random_dense_milp_arrays(60, 30, seed=2)
    p = _ffi.Problem(gpu_ctx, A, b, c)
    t = _ffi.Tree(p, ints, l, u, branch_rule=rule, max_batch=batch, pool_capacity=1 << 16)
    if batch > 1:
        t.set_anchor_mode(True)
        t.set_dive(dive)
    t.set_tree_record(True)
    st = t.solve(mip_gap=0.0, frontier_batch=batch, node_limit=40 if batch == 1 else 1500)
    assert st['status'] == 4 and st['open_nodes'] > 0
    rec = t.tree_records()
    open_ids = np.flatnonzero(rec['flags'] & _ffi.TR_OPEN)
    assert len(open_ids) == st['open_nodes']
    pl, pu, _, pdb = t.peek_open(st['open_nodes'])
    kl, ku = t.node_bounds(open_ids)
    # peek_open lists the nodes in queue order: match them by their rows (the boxes of open nodes are disjoint)
    key = lambda L, U: [bits(L[k]).tobytes() + bits(U[k]).tobytes() for k in range(len(L))]
    want, got = key(pl, pu), key(kl, ku)
    assert len(set(want)) == len(want)
    assert sorted(want) == sorted(got)
    by_row = {r: k for k, r in enumerate(want)}
    for k, r in enumerate(got):   # ... and each carries the bound its record says
        assert np.array_equal(bits([pdb[by_row[r]]]), bits([rec['dual_bound'][open_ids[k]]]))
    t.close()
    p.close()


# ---- 3. a batched search: structure ---------------------------------------------------------------------
def batched(n, m, node_limit, **extra):
    bb = BranchAndBound(generator_model(n, m, 1), PseudoCostBranchNode, pseudo_costs={}, gomory_cuts=False,
                        frontier_batch=256, tree_record=True, mip_gap=0.0, pool_capacity=1 << 20,
                        node_limit=node_limit, **extra)
    bb.solve()
    return bb


_runs = {}


def batched_run(key):
    if key not in _runs:
        n, m, limit = key
        _runs[key] = batched(n, m, limit)
    return _runs[key]


RUNS = [(60, 30, 600), (60, 30, INF), (256, 128, 3000)]


@pytest.mark.parametrize('key', RUNS, ids=['60x30 limit', '60x30 to the end', '256x128 limit'])
def test_batched_search_structure(key):
    bb = batched_run(key)
    tree, rec = bb.tree, bb.tree.rec
    st = bb._native_stats
    if key[2] != INF:
        assert st['open_nodes'] > 0 and bb.status == 'stopped on iterations or time'
    else:
        assert bb.status == 'optimal'
    N = tree.size
    assert N == st['created_nodes'] == bb.tree_record_stats['nodes']
    assert int((rec['lp_status'] >= 0).sum()) == st['evaluated_nodes'] == bb.evaluated_nodes
    assert int((rec['flags'] & _ffi.TR_OPEN != 0).sum()) == st['open_nodes']
    L, U = bb._native.node_bounds(np.arange(N))
    inner = np.flatnonzero(rec['flags'] & _ffi.TR_HAS_CHILDREN)
    assert len(inner) * 2 + 1 == N
    for i in inner:
        kids = tree.get_children(int(i))
        assert len(kids) == 2
        left, right = kids
        var, val = int(rec['bvar'][left]), float(rec['bval'][left])
        assert var == rec['bvar'][right] >= 0 and bits([val]) == bits([rec['bval'][right]])
        assert rec['bdir'][left] == 0 and rec['bdir'][right] == 1
        assert U[left, var] == np.floor(val) and L[right, var] == np.ceil(val)
        others = np.arange(L.shape[1]) != var
        assert np.array_equal(bits(L[left]), bits(L[i])) and np.array_equal(bits(U[right]), bits(U[i]))
        assert np.array_equal(bits(U[left][others]), bits(U[i][others]))
        assert np.array_equal(bits(L[right][others]), bits(L[i][others]))
        # a child's dual_bound is its parent's objective_value
        for kid in kids:
            assert bits([rec['dual_bound'][kid]]) == bits([rec['objective'][i]])
            assert rec['depth'][kid] == rec['depth'][i] + 1
    for i in np.flatnonzero(~(rec['flags'] & _ffi.TR_HAS_CHILDREN).astype(bool)):
        assert tree.get_children(int(i)) == []
    assert tree.subtree_dual_bound(0) == bb.dual_bound
    # The leaves partition the root box.  Leaves here are the nodes without children.  get_leaves(0) is those
    # less the childless nodes the pseudo-cost rule made strong-branching probes from: the Python loop clears
    # is_leaf on such a node (BaseNode._base_branch builds the probe children), the reference does the same,
    # and test 1 holds the record to that.  So get_leaves(0) alone leaves the boxes of those nodes uncovered
    # (measured on the 60 x 30 run to the end: 60 of the 10 000 points), on the Python loop's tree as well.
    childless = (rec['flags'] & _ffi.TR_HAS_CHILDREN) == 0
    probed = (rec['flags'] & _ffi.TR_PROBED) != 0
    assert sorted(tree.get_leaf_ids(0)) == np.flatnonzero(childless & ~probed).tolist()
    assert np.all(rec['lp_status'][childless & probed] >= 0)   # (probes are made from a solved node only)
    leaves = np.flatnonzero(childless)
    lo, up = np.ceil(L[leaves]), np.floor(U[leaves])
    rng = np.random.default_rng(0)
    pts = rng.integers(np.ceil(L[0]).astype(np.int64), np.floor(U[0]).astype(np.int64) + 1, size=(10000, L.shape[1]))
    inside = np.zeros(len(pts), np.int64)
    for k in range(len(leaves)):
        inside += np.all((pts >= lo[k]) & (pts <= up[k]), axis=1)
    assert np.all(inside == 1), (int((inside == 0).sum()), int((inside > 1).sum()))
    # node objects of a sample of the leaves: the record's fields, the kernel's bounds
    for node in tree.get_leaves(0)[:50]:
        assert isinstance(node, PseudoCostBranchNode) and node.is_leaf and node.lineage[0] == 0 and node.lineage[-1] == node.idx
        assert len(node.lineage) == node.depth + 1
        assert np.array_equal(bits(node.lp.variablesLower), bits(L[node.idx]))


# ---- 4. the batched re-solve ------------------------------------------------------------------------
@pytest.mark.parametrize('key', [RUNS[0], RUNS[2]], ids=['60x30', '256x128'])
def test_resolve_agrees_with_the_record_and_is_certified(key):
    bb = batched_run(key)
    rec = bb.tree.rec
    n, m = key[0], key[1]
    A, b, c, l, u, ints = random_dense_milp_arrays(n, m, seed=1)
    feasible = np.flatnonzero(rec['lp_status'] == 0)
    assert len(feasible) >= 200
    ids = np.sort(np.random.default_rng(7).choice(feasible, 200, replace=False))
    res = bb._native.node_solve(ids)
    L, U = bb._native.node_bounds(ids)
    assert np.all(res['status'] == 0)
    Y = np.array([cert.duals_from_basis(A, c, res['vstat'][k]) for k in range(len(ids))])
    M = cert.measure(A, b, c, L, U, res['x'], Y, res['vstat'])
    for k, i in enumerate(ids):
        assert close(res['obj'][k], rec['objective'][i]), (i, res['obj'][k], rec['objective'][i])
        cert.check_optimal(M, k, float(res['obj'][k]), what=f'node {i}')
    infeasible = np.flatnonzero(rec['lp_status'] == 1)   # (the generator's LPs rarely are: see the test below)
    if len(infeasible):
        assert np.all(bb._native.node_solve(infeasible[:200], want_x=False, want_vstat=False)['status'] == 1)
    stats = bb._native.tree_record_stats()
    assert stats['resolved'] >= 200 and stats['query_ms'] > 0


def test_recorded_infeasible_nodes_come_back_infeasible():
    """small_branch without upper bounds: the five infeasible leaves the reference pins (2, 6, 8, 10, 12)."""
    bb = BranchAndBound(std_model('small_branch'), gomory_cuts=False, frontier_batch=1, tree_record=True)
    bb.solve()
    rec = bb.tree.rec
    infeasible = np.flatnonzero(rec['lp_status'] == 1)
    assert infeasible.tolist() == [2, 6, 8, 10, 12]
    res = bb._native.node_solve(np.arange(bb.tree.size))
    assert np.all(res['status'][infeasible] == 1)
    for i in np.flatnonzero(rec['lp_status'] == 0):
        assert res['status'][i] == 0 and close(res['obj'][i], rec['objective'][i]), i


# ---- 5. the disjunctive cut -----------------------------------------------------------------------------
def example_models():
    import json
    table = json.load(open(os.path.join(ROOT, 'golden', 'example_models_optima.json')))['models']
    return [f for k, f in enumerate(sorted(table)) if not (k % 3 or k == 3)]


def test_example_model_selection_is_the_one_of_test_example_models():
    from tests import test_example_models as tem
    assert example_models() == [f for k, (f, _) in enumerate(sorted(tem.TABLE.items())) if not (k % 3 or k == 3)]


@pytest.mark.parametrize('f', example_models())
def test_cglp_from_the_recorded_tree_equals_the_python_trees(f):
    m = MILPInstance(file_name=os.path.join(ROOT, 'golden', 'example_models', f))
    py = BranchAndBound(m, node_limit=8, gomory_cuts=False)
    py.solve()
    bb = BranchAndBound(m, node_limit=8, gomory_cuts=False, frontier_batch=1, tree_record=True)
    bb.solve()
    cp, cn = CutGeneratingLP(py, 0), CutGeneratingLP(bb, 0)
    (pi_p, pi0_p), (pi_n, pi0_n) = cp.solve(), cn.solve()
    assert (pi_p is None) == (pi_n is None)
    if pi_p is None:
        return
    same = close(pi0_p, pi0_n) and all(close(a, b) for a, b in zip(pi_p, pi_n))
    # (alternative optima of the CGLP: the same objective)
    assert same or close(cp.lp.objectiveValue, cn.lp.objectiveValue), (f, cp.lp.objectiveValue, cn.lp.objectiveValue)
    # an inner root: the same disjunction below node 1
    if 1 in py.tree and py.tree.get_node_instances(1).solution is not None:
        ip, inn = CutGeneratingLP(py, 1, depth=2), CutGeneratingLP(bb, 1, depth=2)
        ip.solve(), inn.solve()
        assert close(ip.lp.objectiveValue, inn.lp.objectiveValue), f


def cut_margin_on_leaves(bb, A, b, c_unused):
    """min over the not-infeasible leaves of (min pi.x over the leaf's LP relaxation, by HiGHS) - pi0, with the
    cut and the CGLP.  The disjunction is the tree cut two levels below the root (at most four terms: the engine
    did not solve the CGLP of the seven leaves of the whole Python-loop tree); every leaf of the whole tree
    lies inside one of those terms, so the cut must hold on each of them."""
    cglp = CutGeneratingLP(bb, 0, depth=2)
    pi, pi0 = cglp.solve()
    assert pi is not None, 'the engine did not solve the CGLP'
    assert len(bb.tree.get_leaves(0, depth=2, keep='not infeasible')) <= 4
    pi = np.asarray(pi, np.float64)
    worst = INF
    for leaf in bb.tree.get_leaves(0, keep='not infeasible'):
        lo, up = np.asarray(leaf.lp.variablesLower, np.float64), np.asarray(leaf.lp.variablesUpper, np.float64)
        up = np.where(up >= 1e300, np.inf, up)
        h = linprog(pi, A_ub=-A, b_ub=-b, bounds=list(zip(lo, up)), method='highs')
        if h.status == 2:
            continue   # (an unsolved leaf whose LP is infeasible: the cut says nothing there)
        assert h.status == 0, h.message
        worst = min(worst, h.fun - pi0)
    return worst, pi, pi0, cglp


def test_cut_from_a_batched_tree_is_valid_on_every_leaf():
    """Margin: pi.x >= pi0 - 1e-7 max(1, |pi0|, |pi|_1) on every not-infeasible leaf (PTOL of the contract the
    CGLP itself is solved under), checked on the Python-loop tree's cut first.  The node limits keep the
    CGLP (41 + 100 columns per leaf) inside the LP kernels' 1024 columns."""
    A, b, c, l, u, ints = random_dense_milp_arrays(40, 20, seed=3)
    py = BranchAndBound(generator_model(40, 20, 3), PseudoCostBranchNode, pseudo_costs={}, gomory_cuts=False,
                        node_limit=6)
    py.solve()
    worst, pi, pi0, _ = cut_margin_on_leaves(py, A, b, c)
    margin = 1e-7 * max(1.0, abs(pi0), float(np.abs(pi).sum()))
    print('python-loop tree: worst residual', worst, 'margin', margin)
    assert worst >= -margin
    bb = BranchAndBound(generator_model(40, 20, 3), PseudoCostBranchNode, pseudo_costs={}, gomory_cuts=False,
                        frontier_batch=64, tree_record=True, node_limit=4)
    bb.solve()
    assert bb._native_stats['open_nodes'] > 0
    worst, pi, pi0, cglp = cut_margin_on_leaves(bb, A, b, c)
    margin = 1e-7 * max(1.0, abs(pi0), float(np.abs(pi).sum()))
    print('recorded tree: worst residual', worst, 'margin', margin, 'cglp objective', cglp.lp.objectiveValue)
    assert worst >= -margin
    root = bb.tree.get_node_instances(0)
    assert root is bb.root_node and root.solution is not None
    if cglp.lp.objectiveValue < -1e-7:
        assert float(pi @ root.solution) < pi0   # the root solution violates the cut


# ---- 6. next to the other options -----------------------------------------------------------------------
def tree_by_path(bb):
    """{path of (var, dir) from the root: (lp status, flags, objective bits, inherited bound bits)}."""
    rec = bb.tree.rec
    paths = [()]
    for i in range(1, bb.tree.size):
        paths.append(paths[int(rec['parent'][i])] + ((int(rec['bvar'][i]), int(rec['bdir'][i])),))
    out = {}
    for i, p in enumerate(paths):
        solved = rec['lp_status'][i] in (0, 2)
        out[p] = (int(rec['lp_status'][i]), int(rec['flags'][i]), int(bits([rec['objective'][i]])[0]) if solved else None,
                  int(bits([rec['dual_bound'][i]])[0]), int(bits([rec['bval'][i]])[0]))
    assert len(out) == bb.tree.size
    return out


def run_with(n, m, seed, batch, node_limit=INF, **extra):
    bb = BranchAndBound(generator_model(n, m, seed), PseudoCostBranchNode, pseudo_costs={}, gomory_cuts=False,
                        frontier_batch=batch, tree_record=True, mip_gap=0.0, node_limit=node_limit, **extra)
    bb.solve()
    return bb


def test_host_spill_records_the_tree_of_a_large_pool():
    big = run_with(60, 30, 4, 64, dive=2, pool_capacity=1 << 16)
    small = run_with(60, 30, 4, 64, dive=2, pool_capacity=3 * 64 * 7 * 2 + 1, host_spill=1 << 30)
    assert small.spill_stats['spilled'] > 0 and small.spill_stats['reloaded'] > 0
    assert big.status == small.status == 'optimal'
    assert tree_by_path(big) == tree_by_path(small)


def test_dual_function_records_the_same_tree_and_two_runs_agree():
    plain = run_with(60, 30, 1, 256, pool_capacity=1 << 18)
    again = run_with(60, 30, 1, 256, pool_capacity=1 << 18)
    with_df = run_with(60, 30, 1, 256, pool_capacity=1 << 18, dual_function=True)
    assert plain.status == 'optimal'
    a = tree_by_path(plain)
    assert a == tree_by_path(again)
    for key in plain.tree.rec:   # (two runs of one configuration: identical records, ids included)
        assert np.array_equal(plain.tree.rec[key].view(np.uint8), again.tree.rec[key].view(np.uint8)), key
    assert a == tree_by_path(with_df)
    assert with_df.dual_function_stats['records'] > 0


def test_above_the_register_tiles():
    plain = run_with(300, 150, 0, 256, node_limit=1500, pool_capacity=1 << 18)
    with_df = run_with(300, 150, 0, 256, node_limit=1500, pool_capacity=1 << 18, dual_function=True)
    assert plain.tree.size == plain._native_stats['created_nodes'] > 1
    assert tree_by_path(plain) == tree_by_path(with_df)
    rec = plain.tree.rec
    open_ids = np.flatnonzero(rec['flags'] & _ffi.TR_OPEN)
    pl, pu, _, _ = plain._native.peek_open(len(open_ids))
    kl, ku = plain._native.node_bounds(open_ids)
    rows = lambda L, U: sorted(bits(L[k]).tobytes() + bits(U[k]).tobytes() for k in range(len(L)))
    assert rows(pl, pu) == rows(kl, ku)
    feasible = np.flatnonzero(rec['lp_status'] == 0)[:64]
    res = plain._native.node_solve(feasible, want_x=False, want_vstat=False)
    assert np.all(res['status'] == 0)
    for k, i in enumerate(feasible):
        assert close(res['obj'][k], rec['objective'][i]), (i, res['obj'][k], rec['objective'][i])


def test_engine_refusals(gpu_ctx):
    A, b, c, l, u, ints = random_dense_milp_arrays(20, 10, seed=3)
    p = _ffi.Problem(gpu_ctx, A, b, c)
    t = _ffi.Tree(p, ints, l, u, max_batch=4, pool_capacity=1 << 12)
    with pytest.raises(_ffi.MipxError, match='recording is off'):
        t.tree_records(0, 1)
    with pytest.raises(_ffi.MipxError, match='recording is off'):
        t.node_bounds([0])
    t.solve(frontier_batch=4, max_steps=1)
    with pytest.raises(_ffi.MipxError, match='before the first step'):
        t.set_tree_record(True)
    t.close()
    t = _ffi.Tree(p, ints, l, u, max_batch=4, pool_capacity=1 << 12)
    t.set_tree_record(True)
    t.solve(frontier_batch=4, max_steps=2)
    with pytest.raises(_ffi.MipxError, match='outside the tree'):
        t.node_bounds([10 ** 6])
    l0, u0 = t.node_bounds([0])
    assert np.array_equal(bits(l0[0]), bits(l)) and np.array_equal(bits(u0[0]), bits(u))
    t.close()
    p.close()
