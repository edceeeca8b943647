"""The primal heuristic on the GPU (include/mipx_heur.h): the kernel against the NumPy restatement
(tests/support/heuristic_reference.py) bit for bit, the points it calls feasible certified independently, and the
search with the option on against the search without it and scipy's milp (HiGHS)."""
import functools
import json
import os

import numpy as np
import pytest
from scipy.optimize import Bounds, LinearConstraint, linprog, milp

from simple_mip_solver_amd import (BranchAndBound, MILPInstance, PseudoCostBranchDepthFirstSearchNode,
                                   PseudoCostBranchNode, _ffi)
from simple_mip_solver_amd.generators import random_dense_milp_arrays
from simple_mip_solver_amd.lp import CyLPArray
from simple_mip_solver_amd.utils.primal_heuristic import round_repair_lift
from tests.support import heuristic_reference as ref

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
INF = float('inf')
SHAPES = [(8, 4), (40, 20), (70, 33), (64, 300), (256, 128), (300, 150)]   # n x m
BATCHES = [1, 3, 65]


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def root_vertex(A, b, c, l, u):
    r = linprog(c, A_ub=-A, b_ub=-b, bounds=list(zip(l, u)), method='highs-ds')
    assert r.status == 0, r.message
    return np.asarray(r.x)


def points(n, m, l, u, x0, count=65):
    """The root LP vertex, the box's upper corner (too far from the rows to be repaired within m + n moves), and
    the vertex with half of its coordinates moved by uniform noise of width 0.3, 0.6, 1 or 2, clipped to the box."""
    rng = np.random.default_rng(1000 * n + m)
    X = np.empty((count, n))
    X[0], X[1] = x0, u
    for k in range(2, count):
        w = (0.3, 0.6, 1.0, 2.0)[k % 4]
        X[k] = np.clip(x0 + rng.uniform(-w, w, n) * (rng.random(n) < 0.5), l, u)
    return X


@functools.lru_cache(maxsize=None)
def case(n, m, half=False):
    """One instance per shape, its 65 points and what the restatement makes of them (computed once)."""
    A, b, c, l, u, ints = random_dense_milp_arrays(n, m, seed=1)
    if half:
        ints = list(range(0, n, 2))   # (the odd columns continuous: the sums are no longer exact)
    X = points(n, m, l, u, root_vertex(A, b, c, l, u))
    want = ref.round_repair_lift(A, b, c, l, u, ints, X)
    for a in (A, b, c, l, u, X) + want:
        a.setflags(write=False)
    return A, b, c, l, u, ints, X, want


@pytest.mark.parametrize('n,m', SHAPES)
def test_the_points_exercise_every_outcome(n, m):
    """On the CPU alone: at least a third of a shape's points end feasible, one ends stuck or capped, one needs
    ten or more moves."""
    _, _, _, _, _, _, X, (_, _, status, moves) = case(n, m)
    assert 3 * np.sum(status == ref.FEASIBLE) >= len(X)
    assert np.any((status == ref.STUCK) | (status == ref.CAPPED))
    assert np.any(moves.sum(axis=1) >= 10)


@pytest.mark.parametrize('batch', BATCHES)
@pytest.mark.parametrize('n,m', SHAPES)
def test_kernel_equals_the_restatement_bit_for_bit(n, m, batch, gpu_ctx):
    A, b, c, l, u, ints, X, (Xt, obj, status, moves) = case(n, m)
    p = _ffi.Problem(gpu_ctx, A, b, c)
    got = p.round_repair_batch(X[:batch], l, u, ints)
    p.close()
    assert np.array_equal(got['status'], status[:batch])
    assert np.array_equal(got['moves'], moves[:batch])
    assert np.array_equal(bits(got['x']), bits(Xt[:batch]))
    assert np.array_equal(bits(got['obj']), bits(obj[:batch]))
    for k in np.flatnonzero(got['status'] == ref.FEASIBLE):
        ref.certify(A, b, c, l, u, ints, got['x'][k], got['obj'][k])


@pytest.mark.parametrize('n,m', SHAPES)
def test_kernel_with_continuous_columns(n, m, gpu_ctx):
    """Half of the columns continuous: status and move counts as the restatement's, the point and its objective to
    1e-9 relative, and every point called feasible is."""
    A, b, c, l, u, ints, X, (Xt, obj, status, moves) = case(n, m, True)
    p = _ffi.Problem(gpu_ctx, A, b, c)
    got = p.round_repair_batch(X, l, u, ints)
    p.close()
    assert np.array_equal(got['status'], status) and np.array_equal(got['moves'], moves)
    assert np.all(np.abs(got['x'] - Xt) <= 1e-9 * np.maximum(1.0, np.abs(Xt)))
    assert np.all(np.abs(got['obj'] - obj) <= 1e-9 * np.maximum(1.0, np.abs(obj)))
    cont = np.setdiff1d(np.arange(n), ints)
    assert np.array_equal(bits(got['x'][:, cont]), bits(X[:, cont]))   # (continuous columns are never moved)
    for k in np.flatnonzero(got['status'] == ref.FEASIBLE):
        ref.certify(A, b, c, l, u, ints, got['x'][k], got['obj'][k])


def assert_same(got, want):
    Xt, obj, status, moves = want
    assert np.array_equal(got['status'], status) and np.array_equal(got['moves'], moves)
    assert np.array_equal(bits(got['x']), bits(Xt)) and np.array_equal(bits(got['obj']), bits(obj))


def test_kernel_move_caps_skip_mask_and_clamped_rounding(gpu_ctx):
    A, b, c, l, u, ints, X, _ = case(40, 20)
    p = _ffi.Problem(gpu_ctx, A, b, c)
    X = X[:9]
    # no move at all: the rounded points, capped where a row is violated
    want = ref.round_repair_lift(A, b, c, l, u, ints, X, max_moves=0)
    assert np.any(want[2] == ref.CAPPED) and not want[3].any()
    assert_same(p.round_repair_batch(X, l, u, ints, max_moves=0), want)
    # a cap that hits in the middle of the repair (the corner needs 60 moves), and one that hits in the lift
    want = ref.round_repair_lift(A, b, c, l, u, ints, X, max_moves=3)
    assert want[2][1] == ref.CAPPED and tuple(want[3][1]) == (3, 0)
    assert_same(p.round_repair_batch(X, l, u, ints, max_moves=3), want)
    low = np.zeros((1, 40))   # (the origin satisfies every row: all of its moves are lifts)
    want = ref.round_repair_lift(A, b, c, l, u, ints, low, max_moves=5)
    assert want[2][0] == ref.FEASIBLE and tuple(want[3][0]) == (0, 5)
    assert_same(p.round_repair_batch(low, l, u, ints, max_moves=5), want)
    # the skip mask: skipped points come back as they went in
    skip = np.array([0, 1, 0, 0, 1, 1, 0, 0, 1], np.uint8)
    want = ref.round_repair_lift(A, b, c, l, u, ints, X, skip=skip)
    got = p.round_repair_batch(X, l, u, ints, skip=skip)
    assert_same(got, want)
    assert np.all(got['status'][skip == 1] == ref.SKIPPED) and np.array_equal(bits(got['x'][skip == 1]), bits(X[skip == 1]))
    # points outside the box: the rounding is clamped to the (rounded) bounds, also where the bounds are fractional
    out = np.stack([u + 2.4, l - 1.3, np.where(np.arange(40) % 2, u + 0.7, l - 0.7)])
    lf, uf = l + 0.25, u - 0.25
    for lo, up in ((l, u), (lf, uf)):
        want = ref.round_repair_lift(A, b, c, lo, up, ints, out, max_moves=0)
        assert np.all(want[0] >= np.ceil(lo)) and np.all(want[0] <= np.floor(up))
        assert_same(p.round_repair_batch(out, lo, up, ints, max_moves=0), want)
        assert_same(p.round_repair_batch(out, lo, up, ints), ref.round_repair_lift(A, b, c, lo, up, ints, out))
    p.close()


def test_kernel_ends_stuck_where_no_move_improves(gpu_ctx):
    """x0 + x1 >= 1.5 and -x0 - x1 >= -1.5 over the integers: every unit move trades one violation for the other."""
    A = np.array([[1.0, 1.0], [-1.0, -1.0]]); b = np.array([1.5, -1.5]); c = np.array([1.0, 1.0])
    l, u = np.zeros(2), np.full(2, 5.0)
    X = np.array([[0.6, 0.2], [2.2, 1.9]])
    want = ref.round_repair_lift(A, b, c, l, u, [0, 1], X)
    assert list(want[2]) == [ref.STUCK, ref.STUCK] and tuple(want[3][0]) == (0, 0) and want[3][1][0] > 0
    p = _ffi.Problem(gpu_ctx, A, b, c)
    assert_same(p.round_repair_batch(X, l, u, [0, 1]), want)
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL'):
        p.round_repair_batch(X, l, u, [0, 2])
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL'):
        p.round_repair_batch(X, l, u, [0, 1], tol=-1.0)
    p.close()


def test_example_models_from_their_root_lp_point():
    """The 64 example models: whatever comes back feasible from the root LP point satisfies rows, bounds and
    integrality of the model, with obj = c . x~."""
    from simple_mip_solver_amd.lp import get_backend
    table = json.load(open(os.path.join(HERE, 'golden', 'example_models_optima.json')))['models']
    assert len(table) == 64
    feasible = 0
    for f, rec in sorted(table.items()):
        mdl = MILPInstance(file_name=os.path.join(HERE, 'golden', 'example_models', f))
        rs = mdl.lp._engine_form()
        l, u = mdl.lp._bounds()
        root = get_backend()._problem(rs.A, rs.b, rs.c, rs.key).solve_batch(l[None], u[None])
        assert root['status'][0] == 0, f
        Xt, obj, status, moves = round_repair_lift(mdl, root['x'])
        assert Xt.shape == root['x'].shape and status[0] in (ref.FEASIBLE, ref.STUCK, ref.CAPPED), f
        if status[0] == ref.FEASIBLE:
            feasible += 1
            ref.certify(rs.A, rs.b, rs.c, l, u, sorted(mdl.integerIndices), Xt[0], obj[0])
            assert obj[0] >= rec['milp_opt'] - 1e-6 * max(1.0, abs(rec['milp_opt'])), f   # (no point beats the optimum)
    assert feasible >= 1


# ---- the search -------------------------------------------------------------------------------------------------
def generator_model(n, m, seed, b=None):
    A, b0, c, l, u, ints = random_dense_milp_arrays(n, m, seed=seed)
    return MILPInstance(A=A, b=b0 if b is None else b, c=c, l=l, u=u, sense=['Min', '>='], integerIndices=ints, numVars=n)


@functools.lru_cache(maxsize=None)
def highs_optimum(seed):
    A, b, c, l, u, ints = random_dense_milp_arrays(40, 20, seed=seed)
    h = milp(c, constraints=LinearConstraint(A, lb=b, ub=np.inf), bounds=Bounds(l, u), integrality=np.ones(40),
             options={'mip_rel_gap': 0.0})
    assert h.status == 0
    return float(h.fun)


def search(seed, Node=PseudoCostBranchNode, frontier_batch=64, **kw):
    bb = BranchAndBound(generator_model(40, 20, seed), Node, pseudo_costs={}, gomory_cuts=False, mip_gap=0.0,
                        frontier_batch=frontier_batch, **kw)
    bb.solve()
    return bb


@functools.lru_cache(maxsize=None)
def plain(seed):
    bb = search(seed)
    return bb.status, float(bb.objective_value)


def close(a, b):
    """tests/test_engine_vs_highs_gpu.py's comparison of two optima: 1e-6 relative."""
    return abs(a - b) <= 1e-6 * max(1.0, abs(b))


def certified(bb):
    """bb.solution satisfies rows, bounds and integrality of the root problem, and c . x is bb.objective_value (the
    solution may be a node LP's: rows and objective to 1e-6, integrality to 1e-4, the figures of
    tests/test_engine_vs_highs_gpu.py's comparison)."""
    x = np.asarray(bb.solution)
    rs = bb.root_node.lp._engine_form()
    l, u = bb.root_node.lp._bounds()
    ref.certify(rs.A, rs.b, rs.c, l, u, sorted(bb.model.integerIndices), x, bb.objective_value, tol=1e-6, int_tol=1e-4,
                obj_tol=1e-6)
    return True


def assert_optimal(bb, seed, what=''):
    status, value = plain(seed)
    assert status == 'optimal' and bb.status == status, (what, seed, bb.status)
    assert close(bb.objective_value, value) and close(bb.objective_value, highs_optimum(seed)), \
        (what, seed, bb.objective_value, value, highs_optimum(seed))
    assert certified(bb)


@pytest.mark.parametrize('seed', range(4))
def test_search_with_the_heuristic_finds_the_same_optimum(seed):
    bb = search(seed, primal_heuristic=True)
    assert_optimal(bb, seed)
    st = bb.heuristic_stats
    assert list(st) == list(_ffi.HEUR_STATS_KEYS)
    assert st['incumbents'] >= 1 and st['points'] >= st['feasible'] >= st['incumbents']
    assert st['points'] == st['feasible'] + st['stuck'] + st['capped'] and st['kernel_us'] > 0
    assert search(seed).heuristic_stats is None


@pytest.mark.parametrize('seed', range(4))
def test_an_incumbent_after_the_first_step(seed):
    """Stopped after the root: the plain search holds no incumbent, the search with the heuristic a certified one."""
    off = search(seed, node_limit=1)
    assert off.solution is None and off.objective_value == INF
    on = search(seed, node_limit=1, primal_heuristic=True)
    assert np.isfinite(on.objective_value) and certified(on)
    assert on.objective_value >= highs_optimum(seed) - 1e-6 * max(1.0, abs(highs_optimum(seed)))
    assert on.heuristic_stats['incumbents'] == 1 and on.heuristic_stats['points'] == 1   # (one step, one node: the root)
    assert on._native.stats()['steps'] == off._native.stats()['steps'] == 1


COMBINATIONS = [('tree record', PseudoCostBranchNode, dict(tree_record=True)),
                ('dual function', PseudoCostBranchNode, dict(dual_function=True)),
                ('host spill, small pool', PseudoCostBranchNode, dict(host_spill=1 << 24, frontier_batch=16, pool_capacity=600)),
                ('plunge of 8', PseudoCostBranchNode, dict(dive=8)),
                ('no anchor', PseudoCostBranchNode, dict(anchor=False)),
                ('depth first', PseudoCostBranchDepthFirstSearchNode, dict()),
                ('one node per step', PseudoCostBranchNode, dict(frontier_batch=1)),
                ('one point per step', PseudoCostBranchNode, dict(primal_heuristic=1)),
                ('more points than the batch', PseudoCostBranchNode, dict(primal_heuristic=1000))]


@pytest.mark.parametrize('what,Node,kw', COMBINATIONS, ids=[c[0] for c in COMBINATIONS])
def test_the_same_optimum_beside_the_other_options(what, Node, kw):
    seed = 2
    kw = dict(dict(primal_heuristic=True), **kw)
    bb = search(seed, Node, **kw)
    assert_optimal(bb, seed, what)
    assert bb.heuristic_stats['incumbents'] >= 1
    if 'tree_record' in kw:   # the tree queries still answer
        assert 0 in bb.tree and len(bb.tree.get_leaves(0)) >= 1 and bb.tree_record_stats['nodes'] > 1
    if 'dual_function' in kw:
        assert bb.dual_function_stats['records'] > 0
    if 'host_spill' in kw:
        assert bb.spill_stats is not None
    if what == 'one point per step':
        assert bb.heuristic_stats['points'] <= bb._native.stats()['steps']


def test_every_steps_through_the_c_entry(gpu_ctx):
    A, b, c, l, u, ints = random_dense_milp_arrays(40, 20, seed=1)
    p = _ffi.Problem(gpu_ctx, A, b, c)

    def run(every):
        t = _ffi.Tree(p, ints, l, u, branch_rule='pseudo cost', max_batch=64, pool_capacity=1 << 14)
        t.set_anchor_mode(True)
        t.set_dive(True)
        if every:
            t.set_heuristic(4, every_steps=every, max_moves=60)
        st = t.solve(mip_gap=0.0, frontier_batch=64)
        out = st, t.heuristic_stats(), t.solution()
        t.close()
        return out

    st0, h0, _ = run(0)
    assert st0['status'] == 1 and not any(h0.values())   # (never set: every slot 0)
    for every in (1, 3):
        st, h, x = run(every)
        assert st['status'] == 1 and close(st['primal_bound'], st0['primal_bound']) and close(st['primal_bound'], highs_optimum(1))
        ref.certify(A, b, c, l, u, ints, x, st['primal_bound'], tol=1e-6, int_tol=1e-4, obj_tol=1e-6)
        # 4 points at most in each of the steps that are a multiple of `every`; the root's step is one only for every = 1
        assert 0 < h['points'] <= 4 * (st['steps'] // every)
        if every == 1:
            assert h['incumbents'] >= 1
    p.close()


def test_restart_inherits_the_option():
    src = search(3, tree_record=True, primal_heuristic=5)
    assert_optimal(src, 3)
    b2 = np.asarray(src.model.b, dtype=np.float64) + np.random.default_rng(5).integers(-3, 4, 20)
    new = src.restart(CyLPArray(b2))
    assert new._primal_heuristic == 5
    new.solve()
    h = milp(np.asarray(src.model.lp.objective), constraints=LinearConstraint(np.asarray(src.model.A), lb=b2, ub=np.inf),
             bounds=Bounds(np.asarray(src.model.l), np.asarray(src.model.u)), integrality=np.ones(40), options={'mip_rel_gap': 0.0})
    assert h.status == 0 and new.status == 'optimal' and close(new.objective_value, float(h.fun)) and certified(new)
    assert new.heuristic_stats['points'] > 0
    off = src.restart(CyLPArray(b2), primal_heuristic=None)
    off.solve()
    assert off.heuristic_stats is None and off.status == 'optimal' and close(off.objective_value, float(h.fun))


def test_engine_refusals(gpu_ctx):
    A, b, c, l, u, ints = random_dense_milp_arrays(20, 10, seed=3)
    p = _ffi.Problem(gpu_ctx, A, b, c)
    t = _ffi.Tree(p, ints, l, u, max_batch=4, pool_capacity=1 << 12, cut_params={})
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*not with cut rounds'):
        t.set_heuristic(True)
    t.close()
    t = _ffi.Tree(p, ints, l, u, max_batch=4, pool_capacity=1 << 12)
    for bad in (dict(points=0), dict(every_steps=0), dict(max_moves=0)):
        with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*are positive'):
            t.set_heuristic(**bad)
    t.set_heuristic(True)
    comm = _ffi.Comm(gpu_ctx, 0, 1, allgather=lambda buf: [buf], send=lambda peer, d: None, recv=lambda peer, k: b'')
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*not with the primal heuristic'):
        t.set_comm(comm, 3)
    t.solve(frontier_batch=4, max_steps=1)
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*before the first step'):
        t.set_heuristic(True)
    t.close()
    t = _ffi.Tree(p, ints, l, u, max_batch=4, pool_capacity=1 << 12)
    t.set_comm(comm, 3)
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*not with a communicator'):
        t.set_heuristic(True)
    t.set_comm(None)
    t.close()
    comm.close()
    p.close()


@pytest.mark.parametrize('rule,batch', [('pseudo cost', 1), ('most fractional', 64)])
def test_a_tree_that_never_sets_the_option_is_unchanged(rule, batch, gpu_ctx):
    """Two trees on one instance, the option never set, the trace on: the same trace, node for node, and no
    heuristic counter moves.  (The two configurations whose node order does not depend on when the host finishes a
    step: one node per step, and batches without a pseudo-cost table.)"""
    A, b, c, l, u, ints = random_dense_milp_arrays(40, 20, seed=0)

    def run():
        p = _ffi.Problem(gpu_ctx, A, b, c)   # (a problem of its own: the anchor a search sets stays on its problem)
        t = _ffi.Tree(p, ints, l, u, branch_rule=rule, max_batch=batch, pool_capacity=1 << 16)
        if batch > 1:
            t.set_anchor_mode(True)
            t.set_dive(True)
        t.set_trace(True)
        st = t.solve(mip_gap=0.0, frontier_batch=batch, node_limit=3000)
        out = st, t.trace(), t.heuristic_stats()
        t.close()
        p.close()
        return out

    st1, tr1, h1 = run()
    st2, tr2, h2 = run()
    assert st1['status'] == st2['status'] and st1['primal_bound'] == st2['primal_bound'] and st1['evaluated_nodes'] > 100
    for key in ('evaluated_nodes', 'lp_solved', 'pivots', 'created_nodes', 'steps', 'dives'):
        assert st1[key] == st2[key], key
    for key in ('node_id', 'status', 'branch_var'):
        assert np.array_equal(tr1[key], tr2[key]), key
    assert np.array_equal(bits(tr1['objective']), bits(tr2['objective']))
    assert not any(h1.values()) and not any(h2.values())
