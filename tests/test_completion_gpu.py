"""The completion over the continuous columns on the GPU (include/mipx_complete.h): mipx_complete_batch against the NumPy
restatement around the oracle's node LP (tests/support/completion_reference.py) bit for bit in x, obj, status and
pivots, cold and warm, on the register tiles, at their edge and on the streamed kernel; the edge cases of PREPARE and
FINISH; and searches of a model with continuous columns with the option on against the same searches without it and
scipy's milp (HiGHS)."""
import functools

import numpy as np
import pytest
from scipy.optimize import Bounds, LinearConstraint, milp

from simple_mip_solver_amd import BaseNode, BranchAndBound, MILPInstance, PseudoCostBranchNode, _ffi
from simple_mip_solver_amd.lp import CyLPArray
from simple_mip_solver_amd.utils.completion import complete_continuous
from tests.support import completion_reference as ref
from tests.support import heuristic_reference as heur

gpu = pytest.mark.gpu
KEYS = ('x', 'obj', 'status', 'pivots')


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def assert_same(got, want, what=''):
    """x_out and obj equal bit for bit, status and pivots equal, on every point."""
    print(what, 'status', got['status'][:16], want['status'][:16], 'pivots', got['pivots'][:8], want['pivots'][:8])
    assert np.array_equal(got['status'], want['status']) and np.array_equal(got['pivots'], want['pivots']), what
    assert np.array_equal(bits(got['x']), bits(want['x'])) and np.array_equal(bits(got['obj']), bits(want['obj'])), what


def first(d, k):
    return {key: d[key][:k] for key in KEYS}


# name: (family, n, m, seed) -- half the columns continuous; 8 x 4 and 40 x 20 on the small register tiles (the mixed
# family: some LPs of seed 2 are infeasible), 256 x 128 the largest register tile, 300 x 150 the streamed kernel
SHAPES = {'mixed-8x4': ('mixed', 8, 4, 2), 'mixed-40x20': ('mixed', 40, 20, 2), 'packing-40x20': ('packing', 40, 20, 1),
          'packing-256x128': ('packing', 256, 128, 0), 'packing-300x150': ('packing', 300, 150, 0)}


@functools.lru_cache(maxsize=None)
def case(name):
    """(instance, the 65 rounded points, the basis codes of the LPs they came from, the restatement cold and warm)."""
    family, n, m, seed = SHAPES[name]
    inst = getattr(ref, family)(n, m, seed)
    A, b, c, l, u, ints = inst
    X, V, _, _ = ref.lp_points(inst, seed, 65, 4 if n >= 16 else 2)
    Xt = heur.round_repair_lift(A, b, c, l, u, ints, X)[0]
    lp = ref.oracle_lp(A, b, c)
    return inst, Xt, V, ref.complete(A, b, c, l, u, ints, Xt, lp), ref.complete(A, b, c, l, u, ints, Xt, lp, vstat=V)


@gpu
@pytest.mark.parametrize('name', list(SHAPES))
def test_entry_equals_the_restatement_bit_for_bit(name, gpu_ctx):
    (A, b, c, l, u, ints), Xt, V, cold, warm = case(name)
    assert name == 'mixed-8x4' or np.any(cold['pivots'] != warm['pivots'])   # (the two starts are different solves)
    p = _ffi.Problem(gpu_ctx, A, b, c)
    for k in (1, 3, 65):
        assert_same(p.complete_batch(Xt[:k], l, u, ints), first(cold, k), f'{name} cold batch {k}')
        assert_same(p.complete_batch(Xt[:k], l, u, ints, vstat=V[:k]), first(warm, k), f'{name} warm batch {k}')
    got = p.complete_batch(Xt, l, u, ints, vstat=V)
    p.close()
    for k in np.flatnonzero(got['status'] == ref.COMPLETED):
        heur.certify(A, b, c, l, u, ints, got['x'][k], got['obj'][k], tol=1e-6)
    rest = got['status'] != ref.COMPLETED
    assert np.array_equal(bits(got['x'][rest]), bits(Xt[rest])) and not got['obj'][rest].any()
    if name == 'mixed-40x20':   # (a batch in which some LPs are infeasible)
        assert 0 < int((got['status'] == ref.INFEASIBLE).sum()) < 65 and set(got['status']) == {ref.COMPLETED, ref.INFEASIBLE}
    else:
        assert int((got['status'] == ref.COMPLETED).sum()) > 32


@gpu
def test_edge_cases(gpu_ctx):
    (A, b, c, l, u, ints), Xt, V, cold, warm = case('mixed-40x20')
    n = len(c)
    lp = ref.oracle_lp(A, b, c)
    p = _ffi.Problem(gpu_ctx, A, b, c)
    X = Xt[:9]
    # every column integer: the LP only confirms or refutes the point (the continuous columns of a completed point are
    # not integers: refuted by the integrality test; rounded, the rows decide)
    every = np.arange(n)
    R = np.round(cold['x'][:9])
    R[0] = u   # (inside the bounds and far outside the packing rows)
    want = ref.complete(A, b, c, l, u, every, R, lp)
    assert_same(p.complete_batch(R, l, u, every), want, 'every column integer')
    assert want['status'][0] == ref.INFEASIBLE and set(want['status']) <= {ref.COMPLETED, ref.INFEASIBLE}
    assert ref.complete(A, b, c, l, u, every, cold['x'][:9], lp)['status'].tolist() == \
        p.complete_batch(cold['x'][:9], l, u, every)['status'].tolist()
    # continuous columns with u = +inf
    uinf = u.copy()
    uinf[1::2] = np.inf
    want = ref.complete(A, b, c, l, uinf, ints, X, lp, vstat=V[:9])
    assert_same(p.complete_batch(X, l, uinf, ints, vstat=V[:9]), want, 'u = +inf')
    assert_same(p.complete_batch(X, l, uinf, ints), ref.complete(A, b, c, l, uinf, ints, X, lp), 'u = +inf, cold')
    assert np.any(want['status'] == ref.COMPLETED)
    # a non-integral point, a point outside its rounded bounds and set skip bytes: SKIPPED, unchanged, no pivots
    Y = X.copy()
    Y[1, ints[3]] += 0.25
    Y[4, ints[0]] = u[ints[0]] + 1.0
    skip = np.zeros(9, np.uint8)
    skip[[2, 7]] = 1
    want = ref.complete(A, b, c, l, u, ints, Y, lp, vstat=V[:9], skip=skip)
    got = p.complete_batch(Y, l, u, ints, vstat=V[:9], skip=skip)
    assert_same(got, want, 'skipped points')
    assert got['status'][[1, 2, 4, 7]].tolist() == [ref.SKIPPED] * 4 and not got['pivots'][[1, 2, 4, 7]].any()
    assert np.array_equal(bits(got['x'][[1, 2, 4, 7]]), bits(Y[[1, 2, 4, 7]]))
    assert np.array_equal(got['status'][[0, 3, 5, 6, 8]], cold['status'][[0, 3, 5, 6, 8]])
    # ctol = 0: the recomputed rows must hold exactly; the restatement says which points survive
    want = ref.complete(A, b, c, l, u, ints, Xt, lp, ctol=0.0)
    assert_same(p.complete_batch(Xt, l, u, ints, ctol=0.0), want, 'ctol = 0')
    assert set(want['status']) <= {ref.COMPLETED, ref.INFEASIBLE, ref.REJECTED}
    # a batch of 0 is no launch
    assert len(p.complete_batch(np.zeros((0, n)), l, u, ints)['status']) == 0
    p.close()


@gpu
def test_refusals_of_the_c_entries(gpu_ctx):
    (A, b, c, l, u, ints), Xt, V, cold, warm = case('packing-40x20')
    p = _ffi.Problem(gpu_ctx, A, b, c)
    bad_l, bad_u, int_inf = l.copy(), u.copy(), u.copy()
    bad_l[1] = -np.inf
    bad_u[1] = np.nan
    int_inf[0] = np.inf
    nan_x = Xt[:2].copy()
    nan_x[1, 5] = np.nan
    for args, kw in (((Xt[:2], bad_l, u, ints), {}), ((Xt[:2], l, bad_u, ints), {}), ((Xt[:2], l, int_inf, ints), {}),
                     ((nan_x, l, u, ints), {}), ((Xt[:2], l, u, [0, 0]), {}), ((Xt[:2], l, u, [40]), {}),
                     ((Xt[:2], l, u, ints), dict(ctol=-1.0)), ((Xt[:2], l, u, ints), dict(ctol=np.nan))):
        with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL'):
            p.complete_batch(*args, **kw)
    every = list(range(40))
    t = _ffi.Tree(p, every, l, u, max_batch=16, pool_capacity=1 << 14)
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*mipx_tree_set_heuristic first'):   # without the heuristic
        t.set_completion(True)
    t.set_heuristic(4)
    t.set_completion(True)
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*more points than the completion was set for'):
        t.set_heuristic(8)
    t.set_completion(False)
    t.set_heuristic(8)
    t.set_completion(True)
    t.solve(frontier_batch=16, max_steps=2)
    assert not any(t.completion_stats().values()) and t.heuristic_stats()['points'] > 0   # (no continuous column)
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*before the first step'):   # after a step
        t.set_completion(True)
    t.close()
    p.close()


@gpu
def test_stand_alone_use_on_a_model(gpu_ctx):
    (A, b, c, l, u, ints), Xt, V, cold, warm = case('mixed-40x20')
    mdl = MILPInstance(A=A.copy(), b=b.copy(), c=c.copy(), l=l.copy(), u=u.copy(), sense=['Min', '>='], integerIndices=list(ints),
                       numVars=len(c))
    Xo, obj, status, pivots = complete_continuous(mdl, Xt[:9])
    assert_same(dict(x=Xo, obj=obj, status=status, pivots=pivots), first(cold, 9), 'utility, cold')
    Xo, obj, status, pivots = complete_continuous(mdl, Xt[:9], vstat=V[:9])
    assert_same(dict(x=Xo, obj=obj, status=status, pivots=pivots), first(warm, 9), 'utility, warm')
    one = complete_continuous(mdl, Xt[0], ctol=0.0)
    assert one[0].shape == (1, 40) and one[2][0] in (ref.COMPLETED, ref.REJECTED)


# ---- the search -------------------------------------------------------------------------------------------------
SEED = 0   # (mixed 40 x 20: the restatement completes the root's rounded point and the frozen rounding is stuck; asserted below)


def as_model(A, b, c, l, u, ints):
    return MILPInstance(A=A.copy(), b=b.copy(), c=c.copy(), l=l.copy(), u=u.copy(), sense=['Min', '>='], integerIndices=[int(j) for j in ints],
                        numVars=len(c))


@functools.lru_cache(maxsize=None)
def highs_optimum(family, seed, shift=0):
    A, b, c, l, u, ints = getattr(ref, family)(40, 20, seed)
    b = shifted(b, shift)
    integrality = np.zeros(len(c))
    integrality[ints] = 1
    h = milp(c, constraints=LinearConstraint(A, lb=b, ub=np.inf), bounds=Bounds(l, u), integrality=integrality,
             options={'mip_rel_gap': 0.0})
    assert h.status == 0
    return float(h.fun)


def shifted(b, shift):
    """The right-hand side with its packing rows (the second half) loosened by `shift`."""
    b = np.array(b, dtype=np.float64)
    b[len(b) // 2:] -= shift
    return b


MIP_GAP = 1e-6


def search(family, seed, Node=PseudoCostBranchNode, frontier_batch=64, **kw):
    bb = BranchAndBound(as_model(*getattr(ref, family)(40, 20, seed)), Node, pseudo_costs={}, gomory_cuts=False, mip_gap=MIP_GAP,
                        frontier_batch=frontier_batch, **kw)
    bb.solve()
    return bb


def assert_optimal(bb, family, seed, what='', shift=0):
    want = highs_optimum(family, seed, shift)
    print(what, family, seed, bb.status, bb.objective_value, want, 'nodes', bb.evaluated_nodes, bb.completion_stats, bb.heuristic_stats)
    assert bb.status == 'optimal', (what, bb.status)
    assert abs(bb.objective_value - want) <= (MIP_GAP + 1e-6) * max(1.0, abs(want))
    rs = bb.root_node.lp._engine_form()
    l, u = bb.root_node.lp._bounds()
    heur.certify(rs.A, rs.b, rs.c, l, u, sorted(bb.model.integerIndices), np.asarray(bb.solution), bb.objective_value, tol=1e-6,
                 int_tol=1e-4, obj_tol=1e-6)


@gpu
def test_the_first_step_holds_an_incumbent_only_with_the_option(gpu_ctx):
    inst = ref.mixed(40, 20, SEED)
    A, b, c, l, u, ints = inst
    # what the restatement says of the root: the frozen rounding does not end feasible, its point is completed
    X, V, _, _ = ref.lp_points(inst, SEED, 1)
    xt, _, frozen, _ = heur.round_repair_lift(A, b, c, l, u, ints, X)
    want = ref.complete(A, b, c, l, u, ints, xt, ref.oracle_lp(A, b, c), vstat=V)
    assert frozen[0] != heur.FEASIBLE and want['status'][0] == ref.COMPLETED
    p = _ffi.Problem(gpu_ctx, A, b, c)
    held = {}
    for on in (True, False):
        t = _ffi.Tree(p, [int(j) for j in ints], l, u, branch_rule='pseudo cost', max_batch=64, pool_capacity=1 << 14)
        t.set_heuristic(True)
        if on:
            t.set_completion(True)
        st = t.solve(mip_gap=MIP_GAP, frontier_batch=64, max_steps=1)
        held[on] = (st['has_solution'], st['primal_bound'], t.solution() if st['has_solution'] else None, t.completion_stats(),
                    t.heuristic_stats())
        t.close()
    p.close()
    print(held, want['obj'][0])
    has, primal, x, cs, hs = held[True]
    assert has and abs(primal - want['obj'][0]) <= 1e-9 * max(1.0, abs(primal))
    heur.certify(A, b, c, l, u, ints, x, primal, tol=1e-6)
    assert np.array_equal(x[ints], xt[0][ints])
    assert cs['points'] == cs['completed'] == cs['rescued'] == cs['incumbents'] == 1 and cs['pivots'] == want['pivots'][0]
    assert cs['infeasible'] == cs['failed'] == 0 and cs['kernel_us'] > 0 and hs['feasible'] == 0 and hs['incumbents'] == 1
    assert not held[False][0] and not np.isfinite(held[False][1]) and not any(held[False][3].values())


@gpu
def test_both_searches_end_optimal_at_the_value_of_milp():
    on = search('mixed', SEED, primal_heuristic=True, complete_continuous=True)
    assert_optimal(on, 'mixed', SEED, 'with the option')
    cs, hs = on.completion_stats, on.heuristic_stats
    assert list(cs) == list(_ffi.COMPLETE_STATS_KEYS)
    assert cs['completed'] > 0 and cs['rescued'] > 0 and cs['points'] == hs['points'] > 0
    assert cs['points'] == cs['completed'] + cs['infeasible'] + cs['failed'] and cs['pivots'] > 0 and cs['kernel_us'] > 0
    assert cs['completed'] >= cs['rescued'] and cs['completed'] >= cs['incumbents'] and hs['incumbents'] >= cs['incumbents'] >= 1
    off = search('mixed', SEED, primal_heuristic=True)
    assert_optimal(off, 'mixed', SEED, 'without it')
    assert off.completion_stats is None


@gpu
def test_on_a_pure_integer_model_the_search_is_what_it_was(gpu_ctx):
    """40 x 20, every column integer, most fractional branching (a deterministic order): the same trace with the option
    on as with it off, and zero stats -- nothing is launched."""
    from simple_mip_solver_amd.generators import random_dense_milp_arrays
    A, b, c, l, u, ints = random_dense_milp_arrays(40, 20, seed=1)
    p = _ffi.Problem(gpu_ctx, A, b, c)
    runs = {}
    for on in (False, True):
        t = _ffi.Tree(p, ints, l, u, branch_rule='most fractional', max_batch=64, pool_capacity=1 << 16)
        t.set_trace(True)
        t.set_heuristic(True)
        t.set_local_search(True)
        if on:
            t.set_completion(True)
        st = t.solve(mip_gap=0.0, frontier_batch=64)
        runs[on] = (st, t.trace(), t.heuristic_stats(), t.completion_stats())
        t.close()
    p.close()
    (st0, tr0, hs0, cs0), (st1, tr1, hs1, cs1) = runs[False], runs[True]
    assert _ffi.TREE_STATUS[st1['status']] == 'optimal' and st1['primal_bound'] == st0['primal_bound']
    assert st1['evaluated_nodes'] == st0['evaluated_nodes'] > 1 and len(tr1['node_id']) == len(tr0['node_id']) > 1
    for key in ('node_id', 'status', 'branch_var'):
        assert np.array_equal(tr1[key], tr0[key]), key
    assert np.array_equal(bits(tr1['objective']), bits(tr0['objective']))
    assert {k: v for k, v in hs1.items() if k != 'kernel_us'} == {k: v for k, v in hs0.items() if k != 'kernel_us'}
    assert not any(cs1.values()) and not any(cs0.values())


FAMILIES = [('weighted repair, cube, local search', PseudoCostBranchNode, dict(weighted_repair=True, cube_search=True, local_search=True)),
            ('fix and propagate, cube', PseudoCostBranchNode, dict(fix_propagate=True, cube_search=True)),
            ('most fractional, depth of 8, no anchor', BaseNode, dict(dive=8, anchor=False, local_search=True)),
            ('propagate, reduced cost, host spill', PseudoCostBranchNode,
             dict(propagate=True, reduced_cost=True, host_spill=1 << 24, frontier_batch=16, pool_capacity=600))]


@gpu
@pytest.mark.parametrize('what,Node,kw', FAMILIES, ids=[f[0] for f in FAMILIES])
def test_every_family_goes_through_completion(what, Node, kw):
    bb = search('mixed', SEED, Node, **dict(dict(primal_heuristic=True, complete_continuous=True), **kw))
    assert_optimal(bb, 'mixed', SEED, what)
    cs, hs = bb.completion_stats, bb.heuristic_stats
    assert cs['completed'] > 0 and cs['points'] == cs['completed'] + cs['infeasible'] + cs['failed']
    # the heuristic's slots, and with the cube search its FOUND points: a slot in which the dive or the weighted repair
    # failed holds the LP point again (their OUTPUT) and is skipped, any other slot holds a rounded point and is not
    found = bb.cube_search_stats['found'] if 'cube_search' in kw else 0
    assert hs['feasible'] + found <= cs['points'] <= hs['points'] + found
    if not ({'fix_propagate', 'weighted_repair', 'cube_search'} & set(kw)):
        assert cs['points'] == hs['points']
    # the packing family: the frozen rounding is feasible everywhere and the completion only improves it
    pk = search('packing', 1, Node, **dict(dict(primal_heuristic=True, complete_continuous=True), **kw))
    assert_optimal(pk, 'packing', 1, what)
    assert pk.completion_stats['completed'] > 0 and pk.completion_stats['rescued'] == 0 and pk.completion_stats['infeasible'] == 0


@gpu
def test_restart_inherits_the_option():
    first_ = search('mixed', SEED, tree_record=True, primal_heuristic=True, cube_search=True, complete_continuous=True)
    assert_optimal(first_, 'mixed', SEED, 'recorded')
    b2 = shifted(ref.mixed(40, 20, SEED)[1], 3)
    again = first_.restart(CyLPArray(b2))
    assert again._complete_continuous is True and again._primal_heuristic is True and again._cube_search is True
    again.solve()
    assert_optimal(again, 'mixed', SEED, 'restarted', shift=3)
    assert again.completion_stats['points'] > 0 and again.completion_stats['completed'] > 0
    off = first_.restart(CyLPArray(b2), complete_continuous=None)
    off.solve()
    assert off.completion_stats is None
    assert_optimal(off, 'mixed', SEED, 'restarted without', shift=3)
