"""The pair-move local search on the GPU (include/mipx_lsearch.h): the kernel against the NumPy restatement
(tests/support/local_search_reference.py) bit for bit on the points of tests/support/local_search_cases.py, and the
search with the option on against the search without it and scipy's milp (HiGHS)."""
import functools

import numpy as np
import pytest
from scipy.optimize import Bounds, LinearConstraint, milp

from simple_mip_solver_amd import BranchAndBound, MILPInstance, PseudoCostBranchNode, _ffi
from simple_mip_solver_amd.generators import random_dense_milp_arrays
from simple_mip_solver_amd.lp import CyLPArray
from simple_mip_solver_amd.utils.local_search import pair_search
from tests.support import heuristic_reference as heur
from tests.support import local_search_cases as cases
from tests.support import local_search_reference as ref

gpu = pytest.mark.gpu
BATCHES = [1, 3, 65]
KINDS = ['integer', 'half', 'dyadic']


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def assert_same(got, want, count=None):
    Xo, obj, status, moves = (w[:count] for w in want)
    print('status', got['status'][:16], status[:16], 'moves', got['moves'][:8].tolist(), moves[:8].tolist())
    assert np.array_equal(got['status'], status) and np.array_equal(got['moves'], moves)
    assert np.array_equal(bits(got['x']), bits(Xo)) and np.array_equal(bits(got['obj']), bits(obj))


@pytest.mark.parametrize('n,m', [s for s in cases.SHAPES if s[0] >= 8])
def test_the_points_exercise_every_outcome(n, m):
    """On the restatement alone: the points of a shape include a pair move, a single move, a local optimum reached
    without a move and a capped point -- a kernel that never moves, or never stops, cannot pass the comparison."""
    _, _, _, _, _, _, X, max_moves, (Xo, obj, status, moves) = cases.case(n, m)
    print(n, m, 'max_moves', max_moves, 'status', np.bincount(status, minlength=4), 'singles', moves[:, 0].sum(), 'pairs', moves[:, 1].sum())
    assert np.any(moves[:, 1] > 0) and np.any(moves[:, 0] > 0)
    assert np.any((status == ref.LOCAL_OPT) & (moves.sum(axis=1) == 0))
    assert np.any(status == ref.CAPPED) and np.all(moves.sum(axis=1)[status == ref.CAPPED] == max_moves)
    assert np.all(obj[status != ref.NOT_FEASIBLE] <= X[status != ref.NOT_FEASIBLE] @ cases.instance(n, m)[2] + 1e-9)


@gpu
@pytest.mark.parametrize('batch', BATCHES)
@pytest.mark.parametrize('n,m', list(cases.SHAPES))
def test_kernel_equals_the_restatement_bit_for_bit(n, m, batch, gpu_ctx):
    A, b, c, l, u, ints, X, max_moves, want = cases.case(n, m)
    batch = min(batch, len(X))
    p = _ffi.Problem(gpu_ctx, A, b, c)
    got = p.pair_search_batch(X[:batch], l, u, ints, max_moves=max_moves)
    p.close()
    assert_same(got, want, batch)
    for k in np.flatnonzero(got['status'] != ref.NOT_FEASIBLE):   # (what went in feasible comes out feasible, and no worse)
        heur.certify(A, b, c, l, u, ints, got['x'][k], got['obj'][k])
        assert got['obj'][k] <= float(c @ X[k]) + 1e-9
    same = got['status'] == ref.NOT_FEASIBLE
    assert np.array_equal(bits(got['x'][same]), bits(X[:batch][same]))


@gpu
@pytest.mark.parametrize('kind', KINDS[1:])
@pytest.mark.parametrize('n,m', list(cases.SHAPES))
def test_kernel_on_continuous_columns_and_dyadic_rows(n, m, kind, gpu_ctx):
    """Half of the columns continuous (their values are an LP vertex's: the slacks are no longer exact sums), and rows
    in eighths: still the restatement's bits."""
    A, b, c, l, u, ints, X, max_moves, want = cases.case(n, m, kind)
    p = _ffi.Problem(gpu_ctx, A, b, c)
    got = p.pair_search_batch(X, l, u, ints, max_moves=max_moves)
    p.close()
    assert_same(got, want)
    cont = np.setdiff1d(np.arange(n), ints)
    assert np.array_equal(bits(got['x'][:, cont]), bits(X[:, cont]))   # (continuous columns are never moved)


@gpu
def test_kernel_move_caps_skip_mask_and_aliasing(gpu_ctx):
    A, b, c, l, u, ints, X, _, _ = cases.case(40, 20)
    X = X[:12]
    p = _ffi.Problem(gpu_ctx, A, b, c)
    # no move at all: every point with a candidate is capped, and comes back as it went in
    want = ref.pair_search(A, b, c, l, u, ints, X, max_moves=0)
    assert np.any(want[2] == ref.CAPPED) and np.any(want[2] == ref.LOCAL_OPT) and not want[3].any()
    got = p.pair_search_batch(X, l, u, ints, max_moves=0)
    assert_same(got, want)
    assert np.array_equal(bits(got['x']), bits(X))
    # caps of one and two moves, and the search run to its end
    for cap in (1, 2, 64):
        want = ref.pair_search(A, b, c, l, u, ints, X, max_moves=cap)
        assert_same(p.pair_search_batch(X, l, u, ints, max_moves=cap), want)
        # the output may be the input
        assert_same(p.pair_search_batch(X, l, u, ints, max_moves=cap, in_place=True), want)
    assert not np.any(want[2] == ref.CAPPED) and np.any(want[3].sum(axis=1) > 6)
    # the skip mask: skipped points come back as they went in, with obj 0
    skip = np.array([0, 1, 0, 0, 1, 1, 0, 0, 1, 0, 0, 1], np.uint8)
    want = ref.pair_search(A, b, c, l, u, ints, X, skip=skip)
    for in_place in (False, True):
        got = p.pair_search_batch(X, l, u, ints, skip=skip, in_place=in_place)
        assert_same(got, want)
        assert np.all(got['status'][skip == 1] == ref.SKIPPED) and np.array_equal(bits(got['x'][skip == 1]), bits(X[skip == 1]))
        assert not got['obj'][skip == 1].any()
    # fractional bounds: the rounded bounds decide the room and the check
    lf, uf = l - 0.75, u - 0.25   # (rounded: 0 and 9; a point with a column at 10 is outside)
    want = ref.pair_search(A, b, c, lf, uf, ints, X)
    assert np.any(want[2] == ref.NOT_FEASIBLE) and np.any(want[2] == ref.LOCAL_OPT)
    assert_same(p.pair_search_batch(X, lf, uf, ints), want)
    # fractional and violating points come back untouched
    bad = np.stack([X[0] + 0.5 * (np.arange(40) == 3), u, X[1] - 20.0 * (np.arange(40) == 5)])
    want = ref.pair_search(A, b, c, l, u, ints, bad)
    assert list(want[2]) == [ref.NOT_FEASIBLE] * 3
    got = p.pair_search_batch(bad, l, u, ints)
    assert_same(got, want)
    assert np.array_equal(bits(got['x']), bits(bad))
    # an empty batch is no launch; the refusals
    out = p.pair_search_batch(np.zeros((0, 40)), l, u, ints)
    assert out['status'].shape == (0,) and out['x'].shape == (0, 40)
    for badkw in (dict(integer_indices=[0, 40]), dict(integer_indices=[-1]), dict(integer_indices=[1, 1]), dict(tol=-1.0),
                  dict(max_moves=-1)):
        with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL'):
            p.pair_search_batch(**dict(dict(x=X[:1], l=l, u=u, integer_indices=ints), **badkw))
    p.close()


@gpu
def test_stand_alone_use_on_a_model(gpu_ctx):
    A, b, c, l, u, ints, X, max_moves, want = cases.case(40, 20)
    mdl = MILPInstance(A=A.copy(), b=b.copy(), c=c.copy(), l=l.copy(), u=u.copy(), sense=['Min', '>='], integerIndices=ints,
                       numVars=len(c))
    Xo, obj, status, moves = pair_search(mdl, X, max_moves=max_moves)
    assert_same(dict(x=Xo, obj=obj, status=status, moves=moves), want)
    one = pair_search(mdl, X[1], max_moves=max_moves)
    assert one[0].shape == (1, 40) and one[2][0] == want[2][1]


# ---- the search -------------------------------------------------------------------------------------------------
def generator_model(n, m, seed):
    A, b, c, l, u, ints = random_dense_milp_arrays(n, m, seed=seed)
    return MILPInstance(A=A, b=b, c=c, l=l, u=u, sense=['Min', '>='], integerIndices=ints, numVars=len(c))


@functools.lru_cache(maxsize=None)
def highs_optimum(seed):
    A, b, c, l, u, ints = random_dense_milp_arrays(40, 20, seed=seed)
    h = milp(c, constraints=LinearConstraint(A, lb=b, ub=np.inf), bounds=Bounds(l, u), integrality=np.ones(len(c)),
             options={'mip_rel_gap': 0.0})
    assert h.status == 0
    return float(h.fun)


def search(seed, **kw):
    bb = BranchAndBound(generator_model(40, 20, seed), PseudoCostBranchNode, pseudo_costs={}, gomory_cuts=False, mip_gap=0.0,
                        frontier_batch=64, **kw)
    bb.solve()
    return bb


def close(a, b):
    return abs(a - b) <= 1e-6 * max(1.0, abs(b))


@functools.lru_cache(maxsize=None)
def searched(seed):
    return search(seed, primal_heuristic=True, local_search=True)


@gpu
@pytest.mark.parametrize('seed', range(4))
def test_search_with_the_local_search_finds_the_same_optimum(seed):
    bb = searched(seed)
    st, hs = bb.local_search_stats, bb.heuristic_stats
    print(seed, bb.status, bb.objective_value, highs_optimum(seed), bb.evaluated_nodes, st, hs)
    assert bb.status == 'optimal' and close(bb.objective_value, highs_optimum(seed))
    rs = bb.root_node.lp._engine_form()
    l, u = bb.root_node.lp._bounds()
    heur.certify(rs.A, rs.b, rs.c, l, u, sorted(bb.model.integerIndices), np.asarray(bb.solution), bb.objective_value, tol=1e-6,
                 int_tol=1e-4, obj_tol=1e-6)
    assert list(st) == list(_ffi.LSEARCH_STATS_KEYS) and st['reserved'] == 0
    assert st['points'] == hs['feasible'] > 0 and st['kernel_us'] > 0   # (it runs on the heuristic's feasible points, on all of them)
    assert st['points'] >= st['improved'] >= st['incumbents'] and st['improved'] <= st['single_moves'] + st['pair_moves']
    assert st['capped'] <= st['points'] and hs['incumbents'] >= st['incumbents']
    plain = search(seed, primal_heuristic=True)
    assert plain.local_search_stats is None and plain.status == 'optimal' and close(plain.objective_value, bb.objective_value)


@gpu
def test_the_local_search_improves_points_in_the_search():
    """Summed over the four seeds some point of the heuristic is improved by a pair move."""
    total = {k: sum(searched(seed).local_search_stats[k] for seed in range(4)) for k in _ffi.LSEARCH_STATS_KEYS}
    print(total)
    assert total['improved'] > 0 and total['pair_moves'] > 0


@gpu
def test_move_cap_through_the_keyword_and_the_c_entry(gpu_ctx):
    bb = search(1, primal_heuristic=8, local_search=1)
    st = bb.local_search_stats
    assert bb.status == 'optimal' and close(bb.objective_value, highs_optimum(1))
    assert st['single_moves'] + st['pair_moves'] == st['improved'] and st['capped'] > 0   # (one move per point at most)
    A, b, c, l, u, ints = random_dense_milp_arrays(40, 20, seed=1)
    p = _ffi.Problem(gpu_ctx, A, b, c)
    t = _ffi.Tree(p, ints, l, u, max_batch=16, pool_capacity=1 << 14)
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*mipx_tree_set_heuristic first'):
        t.set_local_search(True)
    t.set_heuristic(4)
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*max_moves is not negative'):
        t.set_local_search(-1)
    t.set_local_search(True)
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*more points than the local search was set for'):
        t.set_heuristic(8)
    t.set_local_search(0)    # off again: the heuristic alone
    t.solve(frontier_batch=16, max_steps=2)
    assert not any(t.local_search_stats().values()) and t.heuristic_stats()['points'] > 0
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*before the first step'):
        t.set_local_search(True)
    t.close()
    t = _ffi.Tree(p, ints, l, u, max_batch=16, pool_capacity=1 << 14)
    t.set_heuristic(4)
    t.set_local_search(5)
    s = t.solve(mip_gap=0.0, frontier_batch=16)
    st = t.local_search_stats()
    assert _ffi.TREE_STATUS[s['status']] == 'optimal' and close(s['primal_bound'], highs_optimum(1))
    assert 0 < st['points'] == t.heuristic_stats()['feasible']
    t.close()
    p.close()


@gpu
def test_restart_inherits_the_option():
    first = search(0, tree_record=True, primal_heuristic=True, local_search=True)
    assert first.status == 'optimal' and first.local_search_stats['points'] > 0
    A, b, c, l, u, ints = random_dense_milp_arrays(40, 20, seed=0)
    b2 = b + np.random.default_rng(5).integers(-3, 4, 20)
    again = first.restart(CyLPArray(b2))
    assert again._local_search is True and again._primal_heuristic is True
    again.solve()
    assert again.status == 'optimal' and again.local_search_stats['points'] > 0
    h = milp(c, constraints=LinearConstraint(A, lb=b2, ub=np.inf), bounds=Bounds(l, u), integrality=np.ones(len(c)),
             options={'mip_rel_gap': 0.0})
    assert h.status == 0 and close(again.objective_value, float(h.fun))
    off = first.restart(CyLPArray(b2), local_search=None)
    off.solve()
    assert off.local_search_stats is None and close(off.objective_value, float(h.fun))


@gpu
@pytest.mark.parametrize('rule,batch', [('pseudo cost', 1), ('most fractional', 64)])
def test_a_tree_that_never_sets_the_option_is_unchanged(rule, batch, gpu_ctx):
    """Two trees on one instance with the heuristic on, the local search never set, the trace on: the same trace, node
    for node, and none of the eight counters moves."""
    A, b, c, l, u, ints = random_dense_milp_arrays(40, 20, seed=0)

    def run():
        p = _ffi.Problem(gpu_ctx, A, b, c)   # (a problem of its own: the anchor a search sets stays on its problem)
        t = _ffi.Tree(p, ints, l, u, branch_rule=rule, max_batch=batch, pool_capacity=1 << 16)
        if batch > 1:
            t.set_anchor_mode(True)
            t.set_dive(True)
        t.set_heuristic(True)
        t.set_trace(True)
        st = t.solve(mip_gap=0.0, frontier_batch=batch, node_limit=3000)
        out = st, t.trace(), t.local_search_stats(), t.heuristic_stats()
        t.close()
        p.close()
        return out

    st1, tr1, h1, hs1 = run()
    st2, tr2, h2, hs2 = run()
    assert st1['status'] == st2['status'] and st1['primal_bound'] == st2['primal_bound'] and st1['evaluated_nodes'] > 100
    for key in ('evaluated_nodes', 'lp_solved', 'pivots', 'created_nodes', 'steps', 'dives'):
        assert st1[key] == st2[key], key
    for key in ('node_id', 'status', 'branch_var'):
        assert np.array_equal(tr1[key], tr2[key]), key
    assert np.array_equal(bits(tr1['objective']), bits(tr2['objective']))
    assert {k: v for k, v in hs1.items() if k != 'kernel_us'} == {k: v for k, v in hs2.items() if k != 'kernel_us'}
    assert list(h1) == list(_ffi.LSEARCH_STATS_KEYS) and len(h1) == 8 and not any(h1.values()) and not any(h2.values())
