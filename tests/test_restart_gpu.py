"""Restarting a recorded search at another right-hand side from its leaves (BranchAndBound.restart,
include/mipx_restart.h).  The comparator is never the restarted search itself: the cold Python loop
(frontier_batch=None), scipy's milp / linprog (HiGHS), the LP certificate helpers, and the queries already pinned
on the SOURCE tree (mipx_tree_records, mipx_tree_node_bounds, find_parameterized_dual_bound)."""
import glob
import os
import re

import numpy as np
import pytest
from scipy.optimize import Bounds, LinearConstraint, linprog, milp

from simple_mip_solver_amd import (BaseNode, BranchAndBound, DepthFirstSearchNode, MILPInstance,
                                   PseudoCostBranchDepthFirstSearchNode, PseudoCostBranchNode, _ffi)
from simple_mip_solver_amd.generators import random_dense_milp_arrays
from simple_mip_solver_amd.lp import CyLPArray
from tests.support import lp_certificate as cert

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.abspath(__file__))
INF = float('inf')
STATUS = {0: 'optimal', 2: 'infeasible', 3: 'unbounded'}   # scipy's status -> BranchAndBound.status

# (Node class, options): both branch rules, both search rules, per-node steps and batches of 256, anchors on
# and off, the plunge on
CONFIGS = [('most fractional, best first, batch 1', BaseNode, dict(frontier_batch=1)),
           ('pseudo cost, best first, batch 256, anchor, dive 2', PseudoCostBranchNode,
            dict(frontier_batch=256, anchor=True, dive=2)),
           ('pseudo cost, depth first, batch 256, no anchor', PseudoCostBranchDepthFirstSearchNode,
            dict(frontier_batch=256, anchor=False, dive=0)),
           ('most fractional, depth first, batch 1', DepthFirstSearchNode, dict(frontier_batch=1))]


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def tol(*values, rel=cert.PTOL):
    """The certificate helpers' tolerance, relative to the figures compared."""
    return rel * max([1.0] + [abs(v) for v in values if np.isfinite(v)])


def node_kwargs(Node):
    return dict(gomory_cuts=False, pseudo_costs={}) if issubclass(Node, PseudoCostBranchNode) else dict(gomory_cuts=False)


def generator_model(n, m, seed, b=None):
    A, b0, c, l, u, ints = random_dense_milp_arrays(n, m, seed=seed)
    return MILPInstance(A=A, b=b0 if b is None else b, c=c, l=l, u=u, sense=['Min', '>='], integerIndices=ints, numVars=n)


def highs(mdl):
    """(status string, optimum) of a MILPInstance by scipy.optimize.milp."""
    A, b = np.asarray(mdl.A), np.asarray(mdl.b, dtype=np.float64)
    con = LinearConstraint(A, lb=b, ub=np.inf) if mdl.sense == '>=' else LinearConstraint(A, lb=-np.inf, ub=b)
    integrality = np.zeros(mdl.numVars)
    integrality[mdl.integerIndices] = 1
    u = np.where(np.asarray(mdl.u) >= 1e300, np.inf, np.asarray(mdl.u))
    h = milp(np.asarray(mdl.lp.objective), constraints=con, bounds=Bounds(np.asarray(mdl.l), u), integrality=integrality,
             options={'mip_rel_gap': 0.0, 'time_limit': 120})
    assert h.status in STATUS, h.message
    return STATUS[h.status], (float(h.fun) if h.status == 0 else INF), (np.asarray(h.x) if h.status == 0 else None)


def cold(mdl):
    """(status, optimum) of the cold Python loop."""
    py = BranchAndBound(mdl, BaseNode, gomory_cuts=False, mip_gap=1e-9)
    py.solve()
    return py.status, float(py.objective_value)


def assert_optimum(bb, want_status, want_value, what):
    """tests/test_engine_vs_highs_gpu.py's comparison: the verdict, and the optimum to 1e-6 relative."""
    assert bb.status == want_status, (what, bb.status, want_status)
    if want_status == 'optimal':
        assert abs(bb.objective_value - want_value) <= 1e-6 * max(1.0, abs(want_value)), (what, bb.objective_value, want_value)
        x = np.asarray(bb.solution)
        rs = bb.root_node.lp._engine_form()
        l, u = bb.root_node.lp._bounds()
        assert np.all(rs.A @ x >= rs.b - 1e-6) and np.all(x >= l - 1e-9) and np.all(x <= u + 1e-9), what
        ints = bb.model.integerIndices
        assert np.all(np.abs(x[ints] - np.round(x[ints])) <= 1e-4), what
        assert abs(float(rs.c @ x) - bb.objective_value) <= 1e-6 * max(1.0, abs(want_value)), what


def seeds_of(native):
    rec = native.tree_records()
    return np.flatnonzero((rec['flags'] & _ffi.TR_HAS_CHILDREN) == 0), rec


def cut_off(mdl, b, x):
    """b with the tightest row of A x >= b raised above A x: x is no longer feasible."""
    A = np.asarray(mdl.A)
    out = np.array(b, dtype=np.float64)
    i = int(np.argmin(A @ x - out))
    out[i] = float(A[i] @ x) + 0.5
    return out


def out_of_range(mdl, b):
    """b with row 0 above what any point of the box reaches: the problem is infeasible."""
    A = np.asarray(mdl.A)
    out = np.array(b, dtype=np.float64)
    out[0] = float(np.sum(np.maximum(A[0] * np.asarray(mdl.l), A[0] * np.asarray(mdl.u)))) + 1.0
    return out


def perturbations(mdl, opt_x, rng):
    """Right-hand sides around mdl.b (rows A x >= b): noise both ways, one that cuts the given optimum off, one
    that is relaxed, one that no point of the box satisfies, and noise again."""
    b = np.asarray(mdl.b, dtype=np.float64)
    m = len(b)
    return [b + rng.uniform(-2, 2, m), cut_off(mdl, b, opt_x), b - rng.uniform(0, 3, m), out_of_range(mdl, b),
            b + rng.uniform(-1, 2, m)]


# ---- 1. the seeds and their pool rows ---------------------------------------------------------------------
@pytest.mark.parametrize('batch,dive,rule,search', [(1, 0, 'most fractional', 'best first'), (64, 2, 'pseudo cost', 'best first'),
                                                    (256, 1, 'pseudo cost', 'best first')])
def test_seeds_are_the_childless_records_and_their_rows_the_lineage_bounds(batch, dive, rule, search, gpu_ctx):
    A, b, c, l, u, ints = random_dense_milp_arrays(60, 30, seed=2)
    p = _ffi.Problem(gpu_ctx, A, b, c)
    src = _ffi.Tree(p, ints, l, u, branch_rule=rule, search_rule=search, max_batch=batch, pool_capacity=1 << 16)
    if batch > 1:
        src.set_anchor_mode(True)
        src.set_dive(dive)
    src.set_tree_record(True)
    st = src.solve(mip_gap=0.0, frontier_batch=batch, node_limit=40 if batch == 1 else 1500)
    want, rec = seeds_of(src)
    assert st['status'] == 4 and np.any(rec['flags'][want] & _ffi.TR_OPEN)   # (stopped early: open nodes among the seeds)
    p2 = _ffi.Problem(gpu_ctx, A, b + np.random.default_rng(1).uniform(-2, 2, len(b)), c)
    t = _ffi.Tree.restart(src, p2)
    seeds = t.restart_seeds()
    assert np.array_equal(seeds, want)
    stats = t.restart_stats()
    n, nv = p.n, p.n + p.m
    assert stats['skeleton'] == st['created_nodes'] and stats['seeds'] == len(want)
    assert stats['device_bytes'] == len(want) * (16 * n + nv) and stats['seed_ms'] > 0
    assert stats['seeds_evaluated'] == stats['seeds_infeasible'] == stats['seeds_integral'] == 0
    first = t.stats()
    assert first['open_nodes'] == len(want) and first['created_nodes'] == st['created_nodes']
    assert first['evaluated_nodes'] == first['lp_solved'] == first['steps'] == 0
    # best first: the seeds sit in the queue in id order, all keyed -inf
    L, U, V, db = t.peek_open(len(want))
    kl, ku = src.node_bounds(want)
    assert np.array_equal(bits(L), bits(kl)) and np.array_equal(bits(U), bits(ku))
    assert np.all(db == -INF)
    assert np.all(V == V[:1]) and int(np.sum(V[0] == cert.BASIC)) == p.m   # one warm-start basis for all: the root's
    # the skeleton: who every node is is kept, what its LP said is reset
    r2 = t.tree_records()
    for key in ('parent', 'bvar', 'bdir', 'depth'):
        assert np.array_equal(r2[key], rec[key]), key
    assert np.array_equal(bits(r2['bval']), bits(rec['bval']))
    assert np.all(r2['lp_status'] == -1) and np.all(r2['dual_bound'] == -INF)
    assert np.array_equal(r2['flags'] & ~_ffi.TR_OPEN, rec['flags'] & _ffi.TR_HAS_CHILDREN)
    src.close()   # (the restarted tree does not lean on its source)
    assert t.solve(mip_gap=1e-9, frontier_batch=batch, node_limit=len(want))['evaluated_nodes'] >= 1
    t.close()
    p2.close()
    p.close()


def test_seed_rows_equal_the_python_loops_node_bounds():
    py = BranchAndBound(generator_model(30, 15, 3), BaseNode, gomory_cuts=False, node_limit=25)
    py.solve()
    bb = BranchAndBound(generator_model(30, 15, 3), BaseNode, gomory_cuts=False, node_limit=25, frontier_batch=1, tree_record=True)
    bb.solve()
    assert bb.evaluated_nodes == py.evaluated_nodes and sorted(py.tree.nodes) == sorted(bb.tree.nodes)
    bb2 = bb.restart(CyLPArray(np.asarray(bb.model.b) + 1.0))
    seeds = bb2._native.restart_seeds()
    assert list(seeds) == sorted(i for i in py.tree.nodes if not py.tree.get_children(i))
    L, U, _, _ = bb2._native.peek_open(len(seeds))
    for k, i in enumerate(seeds):
        node = py.tree.nodes[int(i)].attr['node']
        assert np.array_equal(bits(L[k]), bits(node.lp.variablesLower)), i
        assert np.array_equal(bits(U[k]), bits(node.lp.variablesUpper)), i


# ---- 2. every seed's verdict at the new right-hand side ------------------------------------------------------
@pytest.mark.parametrize('name,Node,opts', CONFIGS[:2], ids=[c[0] for c in CONFIGS[:2]])
def test_every_seed_is_evaluated_and_its_verdict_is_the_lps(name, Node, opts):
    src = BranchAndBound(generator_model(30, 15, 3), Node, tree_record=True, mip_gap=1e-9, **opts, **node_kwargs(Node))
    src.solve()
    b0 = np.asarray(src.model.b, dtype=np.float64)
    bb2 = src.restart(CyLPArray(b0 + np.random.default_rng(11).uniform(-3, 1.5, len(b0))))
    seeds = bb2._native.restart_seeds()
    bb2.solve()
    rec = bb2._native.tree_records()
    st, obj = rec['lp_status'][seeds], rec['objective'][seeds]
    assert np.all(st >= 0), f'seeds left unevaluated: {seeds[st < 0].tolist()}'
    stats = bb2.restart_stats
    assert stats['seeds_evaluated'] == stats['seeds'] == len(seeds)
    assert stats['seeds_infeasible'] == int(np.sum(st == 1))
    assert stats['seeds_integral'] == int(np.sum((rec['flags'][seeds] & _ffi.TR_MIP_FEASIBLE) != 0))
    rs = bb2.root_node.lp._engine_form()
    A, b, c = rs.A, rs.b, rs.c
    L, U = bb2._native.node_bounds(seeds)
    # an independent solve of each leaf LP at the new b: status for status, HiGHS's optimum ...
    for k, i in enumerate(seeds):
        h = linprog(c, A_ub=-A, b_ub=-b, bounds=list(zip(L[k], U[k])), method='highs')
        assert h.status in (0, 2), h.message
        assert int(st[k]) == {0: 0, 2: 1}[h.status], (name, i, int(st[k]), h.status)
        if h.status == 0:
            assert abs(obj[k] - h.fun) <= 1e-6 * max(1.0, abs(h.fun)), (name, i, obj[k], h.fun)
    # ... and the certificate of a re-solve for the recorded objective
    res = bb2._native.node_solve(seeds)
    assert np.array_equal(res['status'], st)
    feasible = np.flatnonzero(st == 0)[:100]   # (the exact arithmetic of the certificates: a bounded number of them)
    Y = np.array([cert.duals_from_basis(A, c, res['vstat'][k]) for k in feasible])
    M = cert.measure(A, b, c, L[feasible], U[feasible], res['x'][feasible], Y, res['vstat'][feasible])
    for q, k in enumerate(feasible):
        cert.check_optimal(M, q, float(obj[k]), what=f'{name} seed {seeds[k]}')
    for k in np.flatnonzero(st == 1)[:25]:
        margin, _ = cert.certify_infeasible(A, b, L[k], U[k], res['vstat'][k])
        assert margin is not None and margin > 0, (name, seeds[k])


# ---- 3. dual function <= the leaves' LPs <= the optimum -----------------------------------------------------
@pytest.mark.parametrize('n,m', [(20, 10), (30, 15)])
def test_sandwich(n, m):
    src = BranchAndBound(generator_model(n, m, 3), PseudoCostBranchNode, pseudo_costs={}, gomory_cuts=False, frontier_batch=64,
                         tree_record=True, dual_function=True, mip_gap=1e-9)
    src.solve()
    assert src.status == 'optimal'
    seeds, _ = seeds_of(src._native)
    L, U = src._native.node_bounds(seeds)
    rs = src.root_node.lp._engine_form()
    rng = np.random.default_rng(5)
    b0 = np.asarray(src.model.b, dtype=np.float64)
    for b in perturbations(src.model, np.asarray(src.solution), rng):
        lower = src.find_parameterized_dual_bound(CyLPArray(b))
        values = []
        for k in range(len(seeds)):
            h = linprog(rs.c, A_ub=-rs.A, b_ub=-b, bounds=list(zip(L[k], U[k])), method='highs')
            assert h.status in (0, 2), h.message
            values.append(h.fun if h.status == 0 else INF)
        leaves = min(values)
        _, optimum, _ = highs(generator_model(n, m, 3, b=b))
        assert lower <= leaves + tol(lower, leaves), (n, m, lower, leaves)
        assert leaves <= optimum + tol(leaves, optimum), (n, m, leaves, optimum)
    assert np.array_equal(b0, np.asarray(src.model.b))


# ---- 4. the optimum ----------------------------------------------------------------------------------------
def value_function_family():
    out = []
    for folder in sorted(glob.glob(os.path.join(ROOT, 'golden', 'example_value_functions', 'instance_*'))):
        files = sorted(glob.glob(os.path.join(folder, 'evaluation_*.mps')), key=lambda f: int(re.search(r'_(\d+).mps', f).group(1)))
        assert len(files) == 40
        out.append(files)
    assert len(out) == 5
    return out


_truth = {}


def truth(key, factory):
    """Cold Python loop and HiGHS on one model, once per module run; they must agree before anything is compared
    with them."""
    if key not in _truth:
        status, value = cold(factory())
        h_status, h_value, h_x = highs(factory())
        assert status == h_status, (key, status, h_status)
        if status == 'optimal':
            assert abs(value - h_value) <= 1e-6 * max(1.0, abs(h_value)), (key, value, h_value)
        _truth[key] = (h_status, h_value, h_x)
    return _truth[key][:2]


@pytest.mark.parametrize('name,Node,opts', CONFIGS, ids=[c[0] for c in CONFIGS])
def test_value_function_instances_by_chained_restarts(name, Node, opts, capsys):
    for files in value_function_family():
        bb = BranchAndBound(MILPInstance(file_name=files[0]), Node, tree_record=True, mip_gap=1e-9, **opts, **node_kwargs(Node))
        bb.solve()
        assert_optimum(bb, *truth(files[0], lambda: MILPInstance(file_name=files[0])), (name, files[0]))
        created = bb._native_stats['created_nodes']
        for f in files[1:]:
            target = MILPInstance(file_name=f)
            bb = bb.restart(target.b)   # (the rows are <=: restart negates b as the dual function does, with its warning)
            assert 'WARNING: your rhs was made negative' in capsys.readouterr().out
            assert bb.status == 'unsolved' and np.array_equal(np.asarray(bb.model.b), -np.asarray(target.b))
            assert bb.restart_stats['skeleton'] == created
            bb.solve()
            assert_optimum(bb, *truth(f, lambda: MILPInstance(file_name=f)), (name, f))
            assert bb.restart_stats['seeds_evaluated'] >= 1
            assert bb._native_stats['created_nodes'] >= created   # (one growing tree)
            created = bb._native_stats['created_nodes']


@pytest.mark.parametrize('n,m', [(20, 10), (30, 15), (40, 20)])
@pytest.mark.parametrize('name,Node,opts', CONFIGS, ids=[c[0] for c in CONFIGS])
def test_generator_instances_at_perturbed_right_hand_sides(name, Node, opts, n, m):
    base = generator_model(n, m, 3)
    status, value = truth((n, m, np.asarray(base.b).tobytes()), lambda: generator_model(n, m, 3))
    # (a source that proved its optimum for the batched rules, one stopped early for the per-node ones)
    limit = dict(node_limit=60) if opts['frontier_batch'] == 1 else {}
    bb = BranchAndBound(base, Node, tree_record=True, mip_gap=1e-9, pool_capacity=1 << 18, **limit, **opts, **node_kwargs(Node))
    bb.solve()
    if not limit:
        assert_optimum(bb, status, value, (name, n, m, 'source'))
    rng = np.random.default_rng(100 + n)
    b = np.asarray(base.b, dtype=np.float64)
    seen, cut_incumbents = set(), 0
    for kind in ('noise', 'incumbent cut off', 'relaxed', 'infeasible', 'noise again'):
        if kind == 'incumbent cut off':   # the incumbent of the search restarted from (HiGHS's optimum where it has none)
            old = np.asarray(bb.solution) if bb.solution is not None else _truth[(n, m, b.tobytes())][2]
            cut_incumbents += bb.solution is not None
            b = cut_off(base, b, old)
            assert np.any(np.asarray(base.A) @ old < b - 0.25)
        elif kind == 'infeasible':
            b = out_of_range(base, b)
        elif kind == 'relaxed':
            b = np.asarray(base.b) - rng.uniform(0, 3, m)
        else:
            b = np.asarray(base.b) + rng.uniform(-2, 2, m)
        bb = bb.restart(CyLPArray(b), node_limit=INF)
        assert np.array_equal(np.asarray(bb.model.b), b)
        bb.solve()
        want = truth((n, m, b.tobytes()), lambda: generator_model(n, m, 3, b=b))
        assert_optimum(bb, *want, (name, n, m, kind))
        seen.add(want[0])
    assert seen == {'optimal', 'infeasible'} and cut_incumbents == 1


# ---- 5. the same right-hand side ----------------------------------------------------------------------------
@pytest.mark.parametrize('name,Node,opts', CONFIGS[:3], ids=[c[0] for c in CONFIGS[:3]])
def test_restart_at_the_same_rhs_ends_with_the_same_optimum(name, Node, opts):
    src = BranchAndBound(generator_model(30, 15, 3), Node, tree_record=True, mip_gap=1e-9, **opts, **node_kwargs(Node))
    src.solve()
    assert src.status == 'optimal'
    bb2 = src.restart(CyLPArray(np.asarray(src.model.b)))
    bb2.solve()
    assert bb2.status == 'optimal'
    assert abs(bb2.objective_value - src.objective_value) <= 1e-9 * max(1.0, abs(src.objective_value))
    c = np.asarray(src.model.lp.objective)
    assert abs(float(c @ bb2.solution) - float(c @ src.solution)) <= 1e-9 * max(1.0, abs(src.objective_value))
    assert bb2.evaluated_nodes >= bb2.restart_stats['seeds']


# ---- 6. the tree of a restarted search ------------------------------------------------------------------------
def test_tree_queries_cover_skeleton_and_new_nodes():
    src = BranchAndBound(generator_model(30, 15, 3), PseudoCostBranchNode, pseudo_costs={}, gomory_cuts=False, frontier_batch=64,
                         tree_record=True, mip_gap=1e-9)
    src.solve()
    N0 = src._native_stats['created_nodes']
    old = src._native.tree_records()
    b = np.asarray(src.model.b, dtype=np.float64) + np.random.default_rng(3).uniform(0, 2.5, 15)   # (tighter: the leaves branch again)
    bb2 = src.restart(CyLPArray(b))
    seeds = bb2._native.restart_seeds()
    assert sorted(bb2.tree.nodes) == [0]   # (until the solve, as for any native search)
    bb2.solve()
    want_status, want_value, _ = highs(generator_model(30, 15, 3, b=b))
    assert_optimum(bb2, want_status, want_value, 'structure')
    rec = bb2._native.tree_records()
    N = len(rec['parent'])
    assert N == bb2._native_stats['created_nodes'] > N0 and len(bb2.tree.nodes) == N
    for key in ('parent', 'bvar', 'bdir', 'depth'):
        assert np.array_equal(rec[key][:N0], old[key]), key
    assert np.array_equal(bits(rec['bval'][:N0]), bits(old['bval']))
    assert np.all(rec['parent'][N0:] >= 0) and np.all(rec['parent'][N0:] < np.arange(N0, N))
    inner = np.setdiff1d(np.arange(N0), seeds)
    assert np.all(rec['lp_status'][inner] == -1)   # skeleton nodes that were no seeds: never solved
    for i in inner[:5]:
        node = bb2.tree.get_node_instances(int(i))
        assert node.lp_feasible is None and node.solution is None and not node.is_leaf
    # new nodes hang under seeds, and the queries see both
    childless = np.flatnonzero((rec['flags'] & _ffi.TR_HAS_CHILDREN) == 0)
    assert np.any(childless >= N0) and np.any(childless < N0)
    leaves = bb2.tree.get_leaf_ids(0)
    assert set(leaves) <= set(childless.tolist()) and any(i >= N0 for i in leaves) and any(i < N0 for i in leaves)
    disj = bb2.tree.get_disjunction(0)
    open_or_feasible = [i for i in leaves if rec['lp_status'][i] in (-1, 0, 2)]
    assert sorted(disj) == sorted(open_or_feasible)
    L, U = bb2._native.node_bounds(sorted(disj))
    for k, i in enumerate(sorted(disj)):
        assert np.array_equal(np.asarray(disj[i][0]), L[k]) and np.array_equal(np.asarray(disj[i][1]), U[k])
    # the optimum lies in one of the disjunction's boxes
    x = np.asarray(bb2.solution)
    assert any(np.all(x >= lo - 1e-9) and np.all(x <= up + 1e-9) for lo, up in disj.values())
    solved = rec['lp_status'][leaves] >= 0
    feas = np.isin(rec['lp_status'][leaves], (0, 2))
    values = np.where(solved, np.where(feas, rec['objective'][leaves], np.inf), rec['dual_bound'][leaves])
    assert bb2.tree.subtree_dual_bound(0) == float(values.min())
    assert bb2.tree.subtree_dual_bound(0) <= want_value + tol(want_value)
    some = [0, int(seeds[0]), N0, N - 1]
    nodes = bb2.tree.get_node_instances(some)
    assert [n.idx for n in nodes] == some
    assert nodes[2].lineage[:-1] == bb2.tree.get_node_instances(int(rec['parent'][N0])).lineage
    assert bb2.tree_record_stats['nodes'] == N


# ---- 7. refusals ------------------------------------------------------------------------------------------
def test_a_pool_too_small_for_the_seeds_is_refused_and_the_source_stays_as_it_was(gpu_ctx):
    A, b, c, l, u, ints = random_dense_milp_arrays(60, 30, seed=2)
    p = _ffi.Problem(gpu_ctx, A, b, c)
    src = _ffi.Tree(p, ints, l, u, branch_rule='most fractional', search_rule='depth first', max_batch=16, pool_capacity=1024)
    src.set_tree_record(True)
    st = src.solve(mip_gap=0.0, frontier_batch=16, node_limit=6000)
    want, before = seeds_of(src)
    assert len(want) + 2 * 16 + 2 > 1024, 'the source must leave more childless records than the pool holds'
    p2 = _ffi.Problem(gpu_ctx, A, b + 1.0, c)
    with pytest.raises(_ffi.MipxError, match=rf'MIPX_ENOMEM.*{len(want)} seeds and the 34 rows a step reserves do not fit the pool of 1024 rows'):
        _ffi.Tree.restart(src, p2)
    after = src.tree_records()
    for key in before:
        assert np.array_equal(bits(before[key]) if before[key].dtype == np.float64 else before[key],
                              bits(after[key]) if after[key].dtype == np.float64 else after[key]), key
    assert src.stats()['created_nodes'] == st['created_nodes']
    more = src.solve(mip_gap=0.0, frontier_batch=16, node_limit=st['evaluated_nodes'] + 32)   # still usable
    assert more['evaluated_nodes'] > st['evaluated_nodes']
    src.close()
    p2.close()
    p.close()


def test_sources_and_problems_the_c_entry_refuses(gpu_ctx):
    A, b, c, l, u, ints = random_dense_milp_arrays(20, 10, seed=3)
    p = _ffi.Problem(gpu_ctx, A, b, c)
    plain = _ffi.Tree(p, ints, l, u, max_batch=4)
    plain.solve(mip_gap=0.0, frontier_batch=4, node_limit=8)
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*the source keeps no record'):
        _ffi.Tree.restart(plain, p)
    plain.close()
    cuts = _ffi.Tree(p, ints, l, u, max_batch=4, cut_params={})
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*(keeps no record|cut rounds)'):
        _ffi.Tree.restart(cuts, p)
    cuts.close()
    src = _ffi.Tree(p, ints, l, u, max_batch=4)
    src.set_tree_record(True)
    src.solve(mip_gap=0.0, frontier_batch=4, node_limit=8)
    A2, b2, c2, _, _, _ = random_dense_milp_arrays(22, 10, seed=3)
    other = _ffi.Problem(gpu_ctx, A2, b2, c2)
    with pytest.raises(_ffi.MipxError, match="MIPX_EINVAL.*the problem's shape differs from the source's"):
        _ffi.Tree.restart(src, other)
    other.close()
    t = _ffi.Tree.restart(src, p)
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*mipx_tree_set_dual_record: not on a restarted tree'):
        t.set_dual_record(1 << 20, p.m, np.arange(p.m), np.ones(p.m))
    assert t.solve(mip_gap=1e-9, frontier_batch=4)['status'] in (1, 2)
    t.close()
    src.close()
    p.close()
