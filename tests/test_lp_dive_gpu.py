"""The LP dive on the GPU (include/mipx_lpdive.h): mipx_lpdive_batch against the NumPy restatement around the oracle's node
LP (tests/support/lp_dive_reference.py) bit for bit in every output -- point, objective, status, rounds, fixings, flips,
pivots -- on the register tiles and on the streamed kernel, with and without codes, with a cutoff, at three round caps
and both rules; and searches of a mixed-integer model with the option on against the same searches without it and
scipy's milp (HiGHS)."""
import functools

import numpy as np
import pytest
from scipy.optimize import Bounds, LinearConstraint, milp

from simple_mip_solver_amd import BaseNode, BranchAndBound, MILPInstance, PseudoCostBranchNode, _ffi
from simple_mip_solver_amd.lp import CyLPArray
from simple_mip_solver_amd.utils.lp_dive import lp_dive
from tests.support import completion_reference as comp
from tests.support import heuristic_reference as heur
from tests.support import lp_dive_reference as ref

gpu = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def assert_same(got, want, what=''):
    """Every output equal on every point: x and obj bit for bit, the integer outputs exactly."""
    print(what, 'status', np.bincount(got['status'], minlength=6), np.bincount(want['status'], minlength=6), 'rounds', got['rounds'][:8],
          want['rounds'][:8], 'pivots', got['pivots'][:8], want['pivots'][:8])
    for key in ('status', 'rounds', 'fixings', 'flips', 'pivots'):
        assert np.array_equal(got[key], want[key]), (what, key, got[key], want[key])
    assert np.array_equal(bits(got['x']), bits(want['x'])) and np.array_equal(bits(got['obj']), bits(want['obj'])), what


def first(d, k):
    return {key: d[key][:k] for key in ref.KEYS}


# name: (family, n, m, seed, points) -- half the columns continuous; 12 x 7 and 40 x 20 on the register tiles (mixed seed
# 1 at 40 x 20: dives that flip and dives that end infeasible), 300 x 30 on the streamed kernel
SHAPES = {'mixed-12x7': ('mixed', 12, 7, 1, 65), 'packing-12x7': ('packing', 12, 7, 0, 65), 'mixed-40x20': ('mixed', 40, 20, 1, 65),
          'packing-40x20': ('packing', 40, 20, 1, 65), 'packing-300x30': ('packing', 300, 30, 0, 8)}


@functools.lru_cache(maxsize=None)
def case(name):
    """(instance, LP points, their codes, their boxes) of one shape, made once."""
    family, n, m, seed, count = SHAPES[name]
    inst = getattr(comp, family)(n, m, seed)
    X, V, L, U = ref.profile_points(inst, seed, count, 4 if n >= 16 else 2)
    return inst, X, V, L, U


@functools.lru_cache(maxsize=None)
def restated(name, rule, warm, max_rounds=64, with_cutoff=False):
    """The restatement's batch, made once per variant; with_cutoff: the median objective of the first round's optimal LPs
    as the cutoff (returned second)."""
    (A, b, c, l, u, ints), X, V, L, U = case(name)
    lp = ref.oracle_lp(A, b, c)
    cutoff = np.inf
    if with_cutoff:
        calls = []

        def recording(Lk, Uk, Vk):
            calls.append(lp(Lk, Uk, Vk))
            return calls[-1]
        ref.dive(A, b, c, L, U, ints, X, recording, vstat=V if warm else None, max_rounds=1, rule=rule)
        cutoff = float(np.median(calls[0]['obj'][calls[0]['status'] == 0]))
    return ref.dive(A, b, c, L, U, ints, X, lp, vstat=V if warm else None, cutoff=cutoff, max_rounds=max_rounds, rule=rule), cutoff


@gpu
@pytest.mark.parametrize('rule', [0, 1], ids=['fractional', 'coefficient'])
@pytest.mark.parametrize('name', list(SHAPES))
def test_entry_equals_the_restatement_bit_for_bit(name, rule, gpu_ctx):
    (A, b, c, l, u, ints), X, V, L, U = case(name)
    B = len(X)
    p = _ffi.Problem(gpu_ctx, A, b, c)
    warm, _ = restated(name, rule, True)
    cold, _ = restated(name, rule, False)
    got = p.lpdive_batch(X, L, U, ints, vstat=V, rule=rule)
    assert_same(got, warm, f'{name} rule {rule} warm batch {B}')
    assert_same(p.lpdive_batch(X, L, U, ints, vstat=V, rule=rule), got, 'two calls')
    assert_same(p.lpdive_batch(X, L, U, ints, rule=rule), cold, f'{name} rule {rule} cold batch {B}')
    if B == 65:   # (64 points, then 1 and 65: a point's dive does not depend on the batch it is in)
        for k in (64, 1):
            assert_same(p.lpdive_batch(X[:k], L[:k], U[:k], ints, vstat=V[:k], rule=rule), first(warm, k), f'{name} warm batch {k}')
    for R in (1, 3):
        want, _ = restated(name, rule, True, R)
        assert_same(p.lpdive_batch(X, L, U, ints, vstat=V, rule=rule, max_rounds=R), want, f'{name} rule {rule} max_rounds {R}')
        assert (want['rounds'] <= R).all() and (R > 1 or (want['status'] == ref.LIMIT).any())   # (the round cap is reached)
    want, cutoff = restated(name, rule, True, 64, True)
    assert_same(p.lpdive_batch(X, L, U, ints, vstat=V, rule=rule, cutoff=cutoff), want, f'{name} rule {rule} cutoff {cutoff}')
    assert (want['status'] == ref.CUTOFF).any()
    p.close()
    # what came back: FEASIBLE points hold, are integral and inside their boxes; every other point is the input
    for k in np.flatnonzero(got['status'] == ref.FEASIBLE):
        heur.certify(A, b, c, L[k], U[k], ints, got['x'][k], got['obj'][k], tol=1e-6)
    rest = got['status'] != ref.FEASIBLE
    assert np.array_equal(bits(got['x'][rest]), bits(X[rest])) and not got['obj'][rest].any()
    assert (got['status'] == ref.FEASIBLE).any()
    if name == 'mixed-40x20':
        assert got['flips'].sum() > 0 and (got['status'] == ref.INFEASIBLE).any()


@gpu
def test_edge_cases_and_refusals(gpu_ctx):
    (A, b, c, l, u, ints), X, V, L, U = case('mixed-40x20')
    n = len(c)
    lp = ref.oracle_lp(A, b, c)
    p = _ffi.Problem(gpu_ctx, A, b, c)
    X, V, L, U = X[:9], V[:9], L[:9], U[:9]
    # every column integer; one integer column
    for cols in (np.arange(n), ints[:1]):
        assert_same(p.lpdive_batch(X, L, U, cols, vstat=V), ref.dive(A, b, c, L, U, cols, X, lp, vstat=V), f'{len(cols)} integer columns')
    # continuous columns with u = +inf
    Uinf = U.copy()
    Uinf[:, 1::2] = np.inf
    assert_same(p.lpdive_batch(X, L, Uinf, ints, vstat=V), ref.dive(A, b, c, L, Uinf, ints, X, lp, vstat=V), 'u = +inf')
    # skipped: a skip byte, an integer column with a fractional bound, one with an infinite bound
    L2, U2 = L.copy(), U.copy()
    L2[1, ints[2]] += 0.5
    U2[4, ints[0]] = np.inf
    skip = np.zeros(9, np.uint8)
    skip[[2, 7]] = 1
    want = ref.dive(A, b, c, L2, U2, ints, X, lp, vstat=V, skip=skip)
    got = p.lpdive_batch(X, L2, U2, ints, vstat=V, skip=skip)
    assert_same(got, want, 'skipped points')
    assert got['status'][[1, 2, 4, 7]].tolist() == [ref.SKIPPED] * 4 and not got['pivots'][[1, 2, 4, 7]].any()
    assert np.array_equal(bits(got['x'][[1, 2, 4, 7]]), bits(X[[1, 2, 4, 7]])) and not got['rounds'][[1, 2, 4, 7]].any()
    # a cutoff below every LP: every dive ends CUTOFF behind its first LP (or INFEASIBLE)
    got = p.lpdive_batch(X, L, U, ints, vstat=V, cutoff=-1e9)
    assert_same(got, ref.dive(A, b, c, L, U, ints, X, lp, vstat=V, cutoff=-1e9), 'cutoff -1e9')
    assert set(got['status']) <= {ref.CUTOFF, ref.INFEASIBLE} and (got['rounds'] <= 2).all()
    assert len(p.lpdive_batch(np.zeros((0, n)), np.zeros((0, n)), np.zeros((0, n)), ints)['status']) == 0
    bad_l, bad_u = L.copy(), U.copy()
    bad_l[0, 1] = -np.inf
    bad_u[0, 1] = np.nan
    for args, kw in (((X, bad_l, U, ints), {}), ((X, L, bad_u, ints), {}), ((X, L, U, [0, 0]), {}), ((X, L, U, [40]), {}),
                     ((X, L, U, ints), dict(max_rounds=0)), ((X, L, U, ints), dict(max_rounds=1025)), ((X, L, U, ints), dict(rule=2)),
                     ((X, L, U, ints), dict(cutoff=np.nan))):
        with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL'):
            p.lpdive_batch(*args, **kw)
    t = _ffi.Tree(p, [int(j) for j in ints], l, u, max_batch=16, pool_capacity=1 << 14)
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*mipx_tree_set_heuristic first'):
        t.set_lpdive(8)
    t.set_heuristic(4)
    for bad in ((1025, 0, 0), (-1, 0, 0), (8, -1, 0), (8, 0, 2)):
        with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL'):
            t.set_lpdive(*bad)
    t.set_lpdive(8)
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*more points than the LP dive was set for'):
        t.set_heuristic(8)
    t.set_lpdive(0)
    t.set_heuristic(8)
    t.set_lpdive(8)
    assert not any(t.lpdive_stats().values())
    t.solve(frontier_batch=16, max_steps=1)
    assert t.lpdive_stats()['points'] > 0
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*before the first step'):
        t.set_lpdive(8)
    t.close()
    p.close()


@gpu
def test_stand_alone_use_on_a_model(gpu_ctx):
    (A, b, c, l, u, ints), X, V, L, U = case('mixed-40x20')
    mdl = as_model(A, b, c, l, u, ints)
    want, _ = restated('mixed-40x20', 1, True)
    out = lp_dive(mdl, X[:9], L[:9], U[:9], vstat=V[:9], rule='coefficient')
    assert_same(dict(zip(ref.KEYS, out)), first(want, 9), 'utility, coefficient rule, warm')
    one = lp_dive(mdl, X[0])   # (the root's point in the root's bounds)
    lp = ref.oracle_lp(A, b, c)
    assert_same(dict(zip(ref.KEYS, one)), ref.dive(A, b, c, l, u, ints, X[:1], lp), 'utility, one point, the root box')


# ---- the search -------------------------------------------------------------------------------------------------
SEED = 1   # (mixed 40 x 20: the seed of tests/test_lp_dive_abi.py's figure -- the completion ends on no point, the dive on 25 of 64)
MIP_GAP = 1e-6


def as_model(A, b, c, l, u, ints):
    return MILPInstance(A=A.copy(), b=b.copy(), c=c.copy(), l=l.copy(), u=u.copy(), sense=['Min', '>='], integerIndices=[int(j) for j in ints],
                        numVars=len(c))


@functools.lru_cache(maxsize=None)
def highs_optimum(family, seed, shift=0):
    A, b, c, l, u, ints = getattr(comp, family)(40, 20, seed)
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


def search(family, seed, Node=PseudoCostBranchNode, frontier_batch=64, **kw):
    bb = BranchAndBound(as_model(*getattr(comp, family)(40, 20, seed)), Node, pseudo_costs={}, gomory_cuts=False, mip_gap=MIP_GAP,
                        frontier_batch=frontier_batch, **kw)
    bb.solve()
    return bb


def assert_optimal(bb, family, seed, what='', shift=0):
    want = highs_optimum(family, seed, shift)
    print(what, family, seed, bb.status, bb.objective_value, want, 'nodes', bb.evaluated_nodes, bb.lp_dive_stats, bb.heuristic_stats)
    assert bb.status == 'optimal', (what, bb.status)
    assert abs(bb.objective_value - want) <= (MIP_GAP + 1e-6) * max(1.0, abs(want))
    rs = bb.root_node.lp._engine_form()
    l, u = bb.root_node.lp._bounds()
    heur.certify(rs.A, rs.b, rs.c, l, u, sorted(bb.model.integerIndices), np.asarray(bb.solution), bb.objective_value, tol=1e-6,
                 int_tol=1e-4, obj_tol=1e-6)


def stepwise(p, inst, on):
    """A tree stepped one step at a time until it holds an incumbent, then to the end: (the step of the first incumbent,
    the dive's stats at that step, the final state, the final stats)."""
    A, b, c, l, u, ints = inst
    t = _ffi.Tree(p, [int(j) for j in ints], l, u, branch_rule='pseudo cost', max_batch=64, pool_capacity=1 << 16)
    t.set_heuristic(True)
    t.set_completion(True)
    if on:
        t.set_lpdive(64)
    st = t.solve(mip_gap=MIP_GAP, frontier_batch=64, max_steps=1)
    while st['status'] == 4 and not np.isfinite(st['primal_bound']):
        st = t.solve(mip_gap=MIP_GAP, frontier_batch=64, max_steps=1)
    first_step, at_first = st['steps'], t.lpdive_stats()
    if st['status'] == 4:
        st = t.solve(mip_gap=MIP_GAP, frontier_batch=64)
    out = (first_step, at_first, st, t.lpdive_stats())
    t.close()
    return out


@gpu
def test_the_dive_brings_the_first_incumbent_no_later(gpu_ctx):
    inst = comp.mixed(40, 20, SEED)
    p = _ffi.Problem(gpu_ctx, inst[0], inst[1], inst[2])
    step_on, at_first, st_on, ds = stepwise(p, inst, True)
    step_off, _, st_off, ds_off = stepwise(p, inst, False)
    p.close()
    want = highs_optimum('mixed', SEED)
    print('first incumbent in step', step_on, 'with the dive,', step_off, 'without; nodes', st_on['evaluated_nodes'], st_off['evaluated_nodes'], ds)
    for st in (st_on, st_off):
        assert _ffi.TREE_STATUS[st['status']] == 'optimal' and abs(st['primal_bound'] - want) <= (MIP_GAP + 1e-6) * max(1.0, abs(want))
    assert step_on <= step_off
    assert list(ds) == list(_ffi.LPDIVE_STATS_KEYS) and not any(ds_off.values())
    assert ds['points'] == ds['feasible'] + ds['infeasible'] + ds['failed'] > 0 and ds['incumbents'] <= ds['feasible']
    assert ds['pivots'] > 0 and ds['moves'] > 0 and ds['kernel_us'] > 0
    # without lp_dive_every the dive runs only while the host holds no incumbent: the counter stops at the first one
    assert ds['points'] == at_first['points'] and ds['pivots'] == at_first['pivots']


@gpu
def test_both_searches_end_optimal_at_the_value_of_milp():
    on = search('mixed', SEED, primal_heuristic=True, complete_continuous=True, lp_dive=True)
    assert_optimal(on, 'mixed', SEED, 'with the option')
    ds = on.lp_dive_stats
    assert list(ds) == list(_ffi.LPDIVE_STATS_KEYS) and ds['points'] > 0
    assert ds['points'] == ds['feasible'] + ds['infeasible'] + ds['failed'] and ds['incumbents'] <= ds['feasible']
    off = search('mixed', SEED, primal_heuristic=True, complete_continuous=True)
    assert_optimal(off, 'mixed', SEED, 'without it')
    assert off.lp_dive_stats is None
    every = search('mixed', SEED, primal_heuristic=True, lp_dive=16, lp_dive_every=2)
    assert_optimal(every, 'mixed', SEED, 'every second step, 16 rounds')
    assert every.lp_dive_stats['points'] > ds['points']


STATS = ('heuristic_stats', 'completion_stats', 'local_search_stats', 'cube_search_stats', 'weighted_repair_stats', 'fix_propagate_stats')


@gpu
def test_with_the_option_off_the_search_is_what_it_was():
    """Most fractional branching (a deterministic order): the same search with lp_dive=None as without the keyword."""
    kw = dict(primal_heuristic=True, complete_continuous=True, local_search=True, cube_search=True, weighted_repair=True)
    a = search('mixed', 0, BaseNode, **kw)
    b = search('mixed', 0, BaseNode, lp_dive=None, lp_dive_every=None, **kw)
    assert a.status == b.status == 'optimal' and a.objective_value == b.objective_value and a.evaluated_nodes == b.evaluated_nodes
    assert np.array_equal(bits(a.solution), bits(b.solution)) and a.lp_dive_stats is None and b.lp_dive_stats is None
    for key in STATS:
        sa, sb = getattr(a, key), getattr(b, key)
        if sa is None or sb is None:
            assert sa is None and sb is None, key
            continue
        assert {k: v for k, v in sa.items() if k != 'kernel_us'} == {k: v for k, v in sb.items() if k != 'kernel_us'}, key


FAMILIES = [('host spill', PseudoCostBranchNode, dict(host_spill=1 << 24, frontier_batch=16, pool_capacity=600)),
            ('depth of 8, no anchor', BaseNode, dict(dive=8, anchor=False)),
            ('tree record', PseudoCostBranchNode, dict(tree_record=True)),
            ('propagate, reduced cost', PseudoCostBranchNode, dict(propagate=True, reduced_cost=True))]


@gpu
@pytest.mark.parametrize('what,Node,kw', FAMILIES, ids=[f[0] for f in FAMILIES])
def test_beside_the_other_options(what, Node, kw):
    on = search('mixed', SEED, Node, **dict(dict(primal_heuristic=True, lp_dive=True), **kw))
    assert_optimal(on, 'mixed', SEED, what)
    assert on.lp_dive_stats['points'] > 0
    off = search('mixed', SEED, Node, **dict(dict(primal_heuristic=True), **kw))
    assert_optimal(off, 'mixed', SEED, what + ', without')
    assert abs(on.objective_value - off.objective_value) <= (MIP_GAP + 1e-6) * max(1.0, abs(off.objective_value))


@gpu
def test_restart_runs_it():
    first_ = search('mixed', SEED, tree_record=True, primal_heuristic=True, lp_dive=True, lp_dive_every=3)
    assert_optimal(first_, 'mixed', SEED, 'recorded')
    b2 = shifted(comp.mixed(40, 20, SEED)[1], 3)
    again = first_.restart(CyLPArray(b2))
    assert again._lp_dive is True and again._lp_dive_every == 3 and again._primal_heuristic is True
    again.solve()
    assert_optimal(again, 'mixed', SEED, 'restarted', shift=3)
    assert again.lp_dive_stats['points'] > 0
    off = first_.restart(CyLPArray(b2), lp_dive=None)
    off.solve()
    assert off.lp_dive_stats is None
    assert_optimal(off, 'mixed', SEED, 'restarted without', shift=3)
