"""The reduced-cost bound tightening on the GPU (include/mipx_rcfix.h): the kernel against the NumPy restatement
(tests/support/reduced_cost_reference.py) bit for bit, and the search with the option on against the search without
it and scipy's milp (HiGHS)."""
import functools

import numpy as np
import pytest
from scipy.optimize import Bounds, LinearConstraint, milp

from simple_mip_solver_amd import (BaseNode, BranchAndBound, MILPInstance,
                                   PseudoCostBranchDepthFirstSearchNode, PseudoCostBranchNode, _ffi)
from simple_mip_solver_amd.generators import random_dense_milp_arrays
from simple_mip_solver_amd.utils.reduced_cost_tightening import tighten_by_reduced_costs
from tests.support import propagation_reference as prop_ref
from tests.support import reduced_cost_reference as ref
from tests.support.heuristic_reference import certify

pytestmark = pytest.mark.gpu
INF = float('inf')
BATCHES = [1, 3, 65]
_own = {}


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def instance(n, m):
    """One instance per shape and its boxes (65; at 1000 x 700 the first 9)."""
    A, b, c, l, u, ints = random_dense_milp_arrays(n, m, seed=0)
    L, U = prop_ref.boxes(A, b, l, u)
    count = ref.boxes_of(n, m)
    return frozen(A, b, c, L[:count].copy(), U[:count].copy()) + (ints,)


def expectation(n, m, Y, feasible):
    """The shape's cutoff for these duals and what the restatement makes of its boxes (computed once per leg)."""
    A, b, c, L, U, ints = instance(n, m)
    cutoff = ref.cutoff_for(ref.tighten(A, b, c, L, U, Y, ints, INF)['z'], feasible)
    exp = ref.tighten(A, b, c, L, U, Y, ints, cutoff)
    frozen(Y, *exp.values())
    return Y, cutoff, exp


@functools.lru_cache(maxsize=None)
def highs_leg(n, m):
    A, b, c, L, U, ints = instance(n, m)
    return expectation(n, m, *ref.highs_duals(A, b, c, L, U))


def own_leg(n, m, ctx):
    """The duals of the project's own batched LP (mipx_lp_solve_batch; zeros where a box is not solved to optimality)."""
    if (n, m) not in _own:
        A, b, c, L, U, ints = instance(n, m)
        p = _ffi.Problem(ctx, A, b, c)
        res = p.solve_batch(L, U)
        p.close()
        solved = res['status'] == 0
        _own[(n, m)] = expectation(n, m, np.where(solved[:, None], res['y'], 0.0), solved)
    return _own[(n, m)]


def assert_same(got, exp, count=None):
    sl = slice(0, count)
    for key in ('status', 'changed'):
        print(key, got[key][:16], exp[key][sl][:16])
        assert np.array_equal(got[key], exp[key][sl]), key
    print('z', got['z'][:4], exp['z'][sl][:4])
    assert np.array_equal(bits(got['z']), bits(exp['z'][sl])), 'z'
    assert np.array_equal(bits(got['l']), bits(exp['l'][sl])) and np.array_equal(bits(got['u']), bits(exp['u'][sl]))


@pytest.mark.parametrize('leg', ['highs', 'own'])
@pytest.mark.parametrize('batch', BATCHES)
@pytest.mark.parametrize('n,m', prop_ref.SHAPES)
def test_kernel_equals_the_restatement_bit_for_bit(n, m, batch, leg, gpu_ctx):
    A, b, c, L, U, ints = instance(n, m)
    Y, cutoff, exp = highs_leg(n, m) if leg == 'highs' else own_leg(n, m, gpu_ctx)
    batch = min(batch, len(L))
    print(leg, 'cutoff', cutoff, 'tightened', int(np.sum(exp['status'] == ref.TIGHTENED)), 'cut off',
          int(np.sum(exp['status'] == ref.CUT_OFF)))
    p = _ffi.Problem(gpu_ctx, A, b, c)
    got = p.reduced_cost_tighten_batch(L[:batch], U[:batch], Y[:batch], ints, cutoff)
    p.close()
    assert_same(got, exp, batch)
    same = got['status'] != ref.TIGHTENED   # (every other node comes back untouched)
    assert np.array_equal(bits(got['l'][same]), bits(L[:batch][same])) and np.array_equal(bits(got['u'][same]), bits(U[:batch][same]))
    if leg == 'highs':   # (tests/test_reduced_cost_abi.py: these inputs tighten, cut off, and leave box 0 alive)
        assert got['status'][0] != ref.CUT_OFF
        if batch == len(L):
            assert np.any(got['status'] == ref.TIGHTENED) and np.any(got['status'] == ref.CUT_OFF)


def test_kernel_on_dyadic_duals(gpu_ctx):
    """y in multiples of 1/8 on integer data: every order of summation gives the same bits
    (tests/test_reduced_cost_abi.py), so this leg holds whatever order the kernel sums in."""
    n, m = 300, 150
    A, b, c, L, U, ints = instance(n, m)
    Y = ref.dyadic_duals(m, len(L))
    z = ref.tighten(A, b, c, L, U, Y, ints, INF)['z']
    p = _ffi.Problem(gpu_ctx, A, b, c)
    for cutoff in (float(np.ceil(np.median(z))), float(np.max(z)) + 50.0, INF):
        exp = ref.tighten(A, b, c, L, U, Y, ints, cutoff)
        print(cutoff, np.bincount(exp['status'], minlength=4))
        assert_same(p.reduced_cost_tighten_batch(L, U, Y, ints, cutoff), exp)
        if np.isfinite(cutoff):
            assert np.any(exp['status'] == ref.TIGHTENED)
    p.close()


def random_case(n, m, seed, count=5):
    rng = np.random.default_rng(seed)
    A = rng.integers(-5, 6, (m, n)).astype(np.float64) * (rng.random((m, n)) < 0.5)
    c = rng.integers(-9, 10, n).astype(np.float64)
    L = rng.integers(0, 4, (count, n)).astype(np.float64)
    U = L + rng.integers(0, 8, (count, n))
    x0 = np.floor((L[0] + U[0]) / 2)
    b = A @ x0 - rng.integers(0, 5, m)
    Y = rng.normal(0.0, 0.4, (count, m)) * (rng.random((count, m)) < 0.6)
    Y[rng.random((count, m)) < 0.05] = np.nan
    return A, b, c, L, U, Y


@pytest.mark.parametrize('n,m,seed', [(5, 1, 6), (1, 3, 5), (257, 6, 263), (1024, 9, 1033), (1024, 1, 1025)])
def test_kernel_at_the_edges_of_its_shapes(n, m, seed, gpu_ctx):
    """One row; one column, one more than a workgroup's threads, and the most a workgroup takes: random rows and
    duals (negative and NaN entries among them), three cutoffs, half of the columns integer."""
    A, b, c, L, U, Y = random_case(n, m, seed=seed)
    ints = np.arange(0, n, 2)
    z = ref.tighten(A, b, c, L, U, Y, ints, INF)['z']
    p = _ffi.Problem(gpu_ctx, A, b, c)
    seen = set()
    for cutoff in (float(np.median(z)) + 3.0, float(np.max(z)) + 40.0, float(np.min(z)) - 1.0):
        exp = ref.tighten(A, b, c, L, U, Y, ints, cutoff)
        seen |= set(exp['status'].tolist())
        got = p.reduced_cost_tighten_batch(L, U, Y, ints, cutoff)
        assert_same(got, exp)
        cont = np.arange(1, n, 2)   # only integer columns move
        assert np.array_equal(bits(got['l'][:, cont]), bits(L[:, cont])) and np.array_equal(bits(got['u'][:, cont]), bits(U[:, cont]))
    p.close()
    assert ref.TIGHTENED in seen and ref.CUT_OFF in seen


def test_kernel_edges(gpu_ctx):
    A = np.array([[1.0, 1.0]]); b = np.array([2.0]); c = np.array([1.0, -1.0])
    p = _ffi.Problem(gpu_ctx, A, b, c)
    L = np.zeros((4, 2)); U = np.array([[5.0, 3.0], [5.0, INF], [INF, 3.0], [INF, INF]])
    Y = np.array([[0.0], [0.0], [0.5], [2.0]])
    for ints in ([0, 1], [1], []):
        for cutoff in (-1.0, -3.5, -3.0 - 5e-7, INF, -INF):
            exp = ref.tighten(A, b, c, L, U, Y, ints, cutoff)
            got = p.reduced_cost_tighten_batch(L, U, Y, ints, cutoff)
            assert_same(got, exp)
            if not np.isfinite(cutoff):   # an infinite cutoff: no bound anywhere
                assert np.all(got['status'] == ref.NO_BOUND)
            assert got['status'][1] == ref.NO_BOUND and got['z'][1] == -INF   # u = +inf under d < 0
            cont = [j for j in (0, 1) if j not in ints]   # only integer columns move
            assert np.array_equal(bits(got['l'][:, cont]), bits(L[:, cont])) and np.array_equal(bits(got['u'][:, cont]), bits(U[:, cont]))
            # the output may be the input
            again = p.reduced_cost_tighten_batch(L, U, Y, ints, cutoff, in_place=True)
            assert_same(again, exp)
    got = p.reduced_cost_tighten_batch(L, U, Y, [0, 1], -1.0)
    assert list(got['status']) == [ref.TIGHTENED, ref.NO_BOUND, ref.TIGHTENED, ref.NO_BOUND]
    assert list(got['u'][0]) == [2.0, 3.0] and list(got['l'][0]) == [0.0, 1.0] and got['changed'][0] == 2
    assert got['u'][2][0] == 5.0 and got['z'][2] == -3.5   # (u = +inf under d > 0 comes down)
    # tolerances of the caller's: dtol above every |d_j| skips every column, tol moves the floor
    assert np.all(p.reduced_cost_tighten_batch(L, U, Y, [0, 1], -1.0, dtol=10.0)['status'][[0, 2]] == ref.UNCHANGED)
    assert_same(p.reduced_cost_tighten_batch(L, U, Y, [0, 1], -1.3, tol=0.5), ref.tighten(A, b, c, L, U, Y, [0, 1], -1.3, tol=0.5))
    # an empty batch is no launch
    out = p.reduced_cost_tighten_batch(np.zeros((0, 2)), np.zeros((0, 2)), np.zeros((0, 1)), [0, 1], -1.0)
    assert out['status'].shape == (0,) and out['l'].shape == (0, 2)
    # the refusals
    for bad in (dict(integer_indices=[0, 2]), dict(integer_indices=[-1]), dict(integer_indices=[1, 1]), dict(tol=-1.0),
                dict(dtol=-1e-9), dict(cutoff=float('nan')), dict(l=np.full((1, 2), -INF)), dict(l=np.full((1, 2), float('nan'))),
                dict(u=np.full((1, 2), float('nan'))), dict(u=np.full((1, 2), -INF))):
        kw = dict(dict(l=L[:1], u=U[:1], y=Y[:1], integer_indices=[0, 1], cutoff=-1.0), **bad)
        with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL'):
            p.reduced_cost_tighten_batch(**kw)
    lib = _ffi.lib()
    one = np.zeros(2); st = np.zeros(1, np.int32)
    args = [p._h, 1, _ffi._ptr(one), _ffi._ptr(one), _ffi._ptr(one), None, 0, -1.0, 1e-6, 1e-9, _ffi._ptr(one), _ffi._ptr(one),
            _ffi._ptr(one), _ffi._ptr(st), _ffi._ptr(st)]
    assert lib.mipx_reduced_cost_tighten_batch(*args) == 0
    for k in (2, 3, 4, 10, 11, 12, 13, 14):   # a null buffer
        assert lib.mipx_reduced_cost_tighten_batch(*[None if q == k else v for q, v in enumerate(args)]) == -1
    assert lib.mipx_reduced_cost_tighten_batch(*[-1 if q == 1 else v for q, v in enumerate(args)]) == -1
    assert lib.mipx_reduced_cost_tighten_batch(*[3 if q == 6 else v for q, v in enumerate(args)]) == -1
    p.close()


def test_stand_alone_use_on_a_model(gpu_ctx):
    A, b, c, l, u, ints = random_dense_milp_arrays(40, 20, seed=0)
    mdl = MILPInstance(A=A, b=b, c=c, l=l, u=u, sense=['Min', '>='], integerIndices=ints, numVars=len(c))
    Y, cutoff, exp = highs_leg(40, 20)
    _, _, _, L, U, _ = instance(40, 20)
    lo, up, z, status, changed = tighten_by_reduced_costs(mdl, L, U, Y, cutoff)
    assert_same(dict(l=lo, u=up, z=z, status=status, changed=changed), exp)
    one = tighten_by_reduced_costs(mdl, L[3], U[3], Y[3], cutoff)
    assert one[0].shape == (1, 40) and one[3][0] == exp['status'][3]


# ---- the search -------------------------------------------------------------------------------------------------
def arrays(family, seed):
    return random_dense_milp_arrays(40, 20, seed=seed) if family == 'packing' else prop_ref.mixed(20, 10, 5, seed)


@functools.lru_cache(maxsize=None)
def highs_optimum(family, seed):
    A, b, c, l, u, ints = arrays(family, seed)
    h = milp(c, constraints=LinearConstraint(A, lb=b, ub=np.inf), bounds=Bounds(l, u), integrality=np.ones(len(c)),
             options={'mip_rel_gap': 0.0})
    assert h.status == 0
    return float(h.fun)


def search(family, seed, Node=PseudoCostBranchNode, frontier_batch=64, **kw):
    A, b, c, l, u, ints = arrays(family, seed)
    mdl = MILPInstance(A=A, b=b, c=c, l=l, u=u, sense=['Min', '>='], integerIndices=ints, numVars=len(c))
    bb = BranchAndBound(mdl, Node, pseudo_costs={}, gomory_cuts=False, mip_gap=0.0, frontier_batch=frontier_batch, **kw)
    bb.solve()
    return bb


@functools.lru_cache(maxsize=None)
def plain(family, seed):
    bb = search(family, seed)
    assert bb.reduced_cost_stats is None
    return bb.status, float(bb.objective_value)


def close(a, b):
    """tests/test_engine_vs_highs_gpu.py's comparison of two optima: 1e-6 relative."""
    return abs(a - b) <= 1e-6 * max(1.0, abs(b))


def certified(bb):
    """bb.solution satisfies rows, bounds and integrality of the root problem, and c . x is bb.objective_value (the
    figures of tests/test_propagation_gpu.py)."""
    rs = bb.root_node.lp._engine_form()
    l, u = bb.root_node.lp._bounds()
    certify(rs.A, rs.b, rs.c, l, u, sorted(bb.model.integerIndices), np.asarray(bb.solution), bb.objective_value, tol=1e-6,
            int_tol=1e-4, obj_tol=1e-6)
    return True


def assert_optimal(bb, family, seed, what=''):
    status, value = plain(family, seed)
    print(what, family, seed, bb.status, bb.objective_value, value, highs_optimum(family, seed), bb.reduced_cost_stats)
    assert status == 'optimal' and bb.status == status, (what, seed, bb.status)
    assert close(bb.objective_value, value) and close(bb.objective_value, highs_optimum(family, seed)), \
        (what, seed, bb.objective_value, value, highs_optimum(family, seed))
    assert certified(bb)
    st = bb.reduced_cost_stats
    assert list(st) == list(_ffi.RCFIX_STATS_KEYS) and st['reserved'] == 0
    assert st['nodes'] >= st['tightened'] + st['cut_off'] + st['no_bound'] and st['bounds_changed'] >= st['tightened']
    assert (st['launches'] > 0) == (st['nodes'] > 0) == (st['kernel_us'] > 0) and st['nodes'] >= st['launches']


@functools.lru_cache(maxsize=None)
def tightened_search(family, seed, heuristic=False):
    return search(family, seed, reduced_cost=True, **(dict(primal_heuristic=True) if heuristic else {}))


@pytest.mark.parametrize('seed', range(4))
@pytest.mark.parametrize('family', ['packing', 'mixed'])
def test_search_with_the_tightening_finds_the_same_optimum(family, seed):
    bb = tightened_search(family, seed)
    assert_optimal(bb, family, seed)
    assert bb.reduced_cost_stats['kernel_us'] > 0
    assert search(family, seed).reduced_cost_stats is None


@pytest.mark.parametrize('family', ['packing', 'mixed'])
def test_the_tightening_moves_bounds_in_the_search(family):
    """Summed over the four seeds of a family some node is tightened; with the primal heuristic, which gives the
    cutoff an incumbent from step one, on every seed."""
    alone = [tightened_search(family, seed).reduced_cost_stats for seed in range(4)]
    print([st['tightened'] for st in alone])
    assert sum(st['tightened'] for st in alone) > 0
    for seed in range(4):
        bb = tightened_search(family, seed, heuristic=True)
        assert_optimal(bb, family, seed, 'primal heuristic')
        assert bb.reduced_cost_stats['tightened'] > 0 and bb.heuristic_stats['incumbents'] >= 1, seed


COMBINATIONS = [('host spill, small pool', PseudoCostBranchNode, dict(host_spill=1 << 24, frontier_batch=16, pool_capacity=600)),
                ('plunge of 8', PseudoCostBranchNode, dict(dive=8)),
                ('no anchor', PseudoCostBranchNode, dict(anchor=False)),
                ('depth first', PseudoCostBranchDepthFirstSearchNode, dict()),
                ('most fractional', BaseNode, dict()),
                ('one node per step', PseudoCostBranchNode, dict(frontier_batch=1)),
                ('primal heuristic', PseudoCostBranchNode, dict(primal_heuristic=True)),
                ('propagation', PseudoCostBranchNode, dict(propagate=True))]


@pytest.mark.parametrize('family,seed', [('packing', 2), ('mixed', 1)])
@pytest.mark.parametrize('what,Node,kw', COMBINATIONS, ids=[c[0] for c in COMBINATIONS])
def test_the_same_optimum_beside_the_other_options(what, Node, kw, family, seed):
    bb = search(family, seed, Node, **dict(dict(reduced_cost=True), **kw))
    assert_optimal(bb, family, seed, what)
    assert bb.reduced_cost_stats['nodes'] > 0   # (an incumbent is found before the search ends, and nodes branch after it)
    if 'host_spill' in kw:
        assert bb.spill_stats is not None
    if 'primal_heuristic' in kw:
        assert bb.heuristic_stats['incumbents'] >= 1
    if 'propagate' in kw:
        assert bb.propagation_stats['nodes'] > 0


def test_engine_refusals(gpu_ctx):
    A, b, c, l, u, ints = random_dense_milp_arrays(20, 10, seed=3)
    p = _ffi.Problem(gpu_ctx, A, b, c)
    t = _ffi.Tree(p, ints, l, u, max_batch=4, pool_capacity=1 << 12, cut_params={})
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*mipx_tree_set_reduced_cost: not with cut rounds'):
        t.set_reduced_cost(True)
    t.close()
    t = _ffi.Tree(p, ints, l, u, max_batch=4, pool_capacity=1 << 12)
    t.set_reduced_cost(True)
    comm = _ffi.Comm(gpu_ctx, 0, 1, allgather=lambda buf: [buf], send=lambda peer, d: None, recv=lambda peer, k: b'')
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*mipx_tree_set_comm: not with the reduced-cost tightening'):
        t.set_comm(comm, 3)
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*mipx_tree_set_tree_record: not with the reduced-cost tightening'):
        t.set_tree_record(True)
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*mipx_tree_set_dual_record: not with the reduced-cost tightening'):
        t.set_dual_record(1 << 20, 10, np.arange(10, dtype=np.int32), np.ones(10))
    t.solve(frontier_batch=4, max_steps=1)
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*before the first step'):
        t.set_reduced_cost(True)
    t.close()
    t = _ffi.Tree(p, ints, l, u, max_batch=4, pool_capacity=1 << 12)
    t.set_comm(comm, 3)
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*mipx_tree_set_reduced_cost: not with a communicator'):
        t.set_reduced_cost(True)
    t.set_comm(None)
    t.close()
    t = _ffi.Tree(p, ints, l, u, max_batch=4, pool_capacity=1 << 12)
    t.set_tree_record(True)
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*mipx_tree_set_reduced_cost: not with the tree record'):
        t.set_reduced_cost(True)
    t.close()
    t = _ffi.Tree(p, ints, l, u, max_batch=4, pool_capacity=1 << 12)
    t.set_dual_record(1 << 20, 10, np.arange(10, dtype=np.int32), np.ones(10))
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*mipx_tree_set_reduced_cost: not with the dual function'):
        t.set_reduced_cost(True)
    t.close()
    comm.close()
    p.close()


@pytest.mark.parametrize('rule,batch', [('pseudo cost', 1), ('most fractional', 64)])
def test_a_tree_that_never_sets_the_option_is_unchanged(rule, batch, gpu_ctx):
    """Two trees on one instance, the option never set, the trace on: the same trace, node for node, and none of the
    eight counters moves.  (The two configurations whose node order does not depend on when the host finishes a
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
        out = st, t.trace(), t.reduced_cost_stats()
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
    assert list(h1) == list(_ffi.RCFIX_STATS_KEYS) and len(h1) == 8 and not any(h1.values()) and not any(h2.values())
