"""The weighted row repair on the GPU (include/mipx_wrepair.h): the kernel against the NumPy restatement
(tests/support/weighted_repair_reference.py) bit for bit on the cases of that module, and the search with the option on
against the search without it and scipy's milp (HiGHS)."""
import functools

import numpy as np
import pytest
from scipy.optimize import Bounds, LinearConstraint, milp

from simple_mip_solver_amd import BaseNode, BranchAndBound, MILPInstance, PseudoCostBranchNode, _ffi
from simple_mip_solver_amd.generators import random_dense_milp_arrays
from simple_mip_solver_amd.lp import CyLPArray
from simple_mip_solver_amd.utils.weighted_repair import weighted_repair
from tests.support import heuristic_reference as heur
from tests.support import weighted_repair_reference as ref
from tests.support.fix_propagate_reference import lp_points
from tests.support.propagation_reference import mixed

gpu = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def assert_same(got, want, count=None):
    """x~ and obj equal bit for bit, status and both counts equal, on every point."""
    w = {k: v[:count] for k, v in want.items()}
    print('status', got['status'][:16], w['status'][:16], 'counts', got['counts'][:6].tolist(), w['counts'][:6].tolist())
    assert np.array_equal(got['status'], w['status']) and np.array_equal(got['counts'], w['counts'])
    assert np.array_equal(bits(got['x']), bits(w['x'])) and np.array_equal(bits(got['obj']), bits(w['obj']))


@gpu
@pytest.mark.parametrize('name', list(ref.CASES))
def test_kernel_equals_the_restatement_bit_for_bit(name, gpu_ctx):
    A, b, c, l, u, ints, X, max_steps, tol, skip, gate, want = ref.case(name)
    p = _ffi.Problem(gpu_ctx, A, b, c)
    got = p.weighted_repair_batch(X, l, u, ints, tol=tol, max_steps=max_steps, skip=skip, gate=gate)
    k1 = 1 if gate is not None else 0   # (a batch of 1, of a point the gate lets through)
    one = p.weighted_repair_batch(X[k1:k1 + 1], l, u, ints, tol=tol, max_steps=max_steps)
    three = p.weighted_repair_batch(X[:3], l, u, ints, tol=tol, max_steps=max_steps, gate=None if gate is None else gate[:3])
    p.close()
    assert_same(got, want)
    assert_same(one, {k: v[k1:k1 + 1] for k, v in want.items()})
    if skip is None:
        assert_same(three, want, 3)
    for k in np.flatnonzero(got['status'] == ref.FEASIBLE):
        heur.certify(A, b, c, l, u, ints, got['x'][k], got['obj'][k], tol=tol)
    same = got['status'] != ref.FEASIBLE
    assert np.array_equal(bits(got['x'][same]), bits(X[same])) and not got['obj'][same].any()


@gpu
def test_kernel_on_lp_points_where_the_rounding_is_stuck(gpu_ctx):
    """The points of the CPU condition (64 LP points of mixed(40, 20, 10, 2)): bit for bit, all feasible, and gated by
    the rounding heuristic's own status exactly the points it did not end feasible on are run."""
    A, b, c, l, u, ints = mixed(40, 20, 10, 2)
    X = lp_points(A, b, c, l, u, ints, 64, seed=2)
    p = _ffi.Problem(gpu_ctx, A, b, c)
    h = p.round_repair_batch(X, l, u, ints)
    got = p.weighted_repair_batch(X, l, u, ints)
    gated = p.weighted_repair_batch(X, l, u, ints, gate=h['status'])
    p.close()
    want = ref.weighted_repair(A, b, c, l, u, ints, X)
    assert_same(got, want)
    assert np.all(got['status'] == ref.FEASIBLE) and got['counts'].sum(axis=1).max() <= 64 and got['counts'][:, 1].max() > 0
    assert_same(gated, ref.weighted_repair(A, b, c, l, u, ints, X, gate=h['status']))
    assert np.array_equal(gated['status'] == ref.SKIPPED, h['status'] == heur.FEASIBLE) and np.any(h['status'] == heur.STUCK)


@gpu
def test_kernel_caps_tolerances_orders_and_refusals(gpu_ctx):
    A, b, c, l, u, ints, X, _, _, _, _, _ = ref.case('mixed-40x20')
    X = X[:12]
    p = _ffi.Problem(gpu_ctx, A, b, c)
    for kw in (dict(max_steps=0), dict(max_steps=1), dict(max_steps=7), dict(tol=0.0), dict(tol=1e-7), dict(tol=1e-3)):
        want = ref.weighted_repair(A, b, c, l, u, ints, X, **kw)
        assert_same(p.weighted_repair_batch(X, l, u, ints, **kw), want)
        if kw.get('max_steps', 99) < 1:   # (a point whose rounding breaks no row is feasible under any cap)
            assert set(want['status']) <= {ref.CAPPED, ref.FEASIBLE} and not want['counts'].any()
    # fractional bounds are rounded as the heuristic rounds them; integer columns given in another order
    lf, uf = l - 0.75, u - 0.25   # (rounded: 0 and 9)
    want = ref.weighted_repair(A, b, c, lf, uf, ints, np.clip(X, lf, uf))
    assert np.any(want['status'] == ref.FEASIBLE)
    assert_same(p.weighted_repair_batch(np.clip(X, lf, uf), lf, uf, ints[::-1]), want)
    # an upper bound of +inf
    ui = u.copy(); ui[::3] = np.inf
    assert_same(p.weighted_repair_batch(X, l, ui, ints, max_steps=60), ref.weighted_repair(A, b, c, l, ui, ints, X, max_steps=60))
    # no integer column at all: no candidate, so a point with a broken row only bumps, to the cap
    want = ref.weighted_repair(A, b, c, l, u, [], X, max_steps=5)
    assert set(want['status']) <= {ref.FEASIBLE, ref.CAPPED} and not want['counts'][:, 0].any()
    assert_same(p.weighted_repair_batch(X, l, u, [], max_steps=5), want)
    # an empty batch is no launch; the refusals
    out = p.weighted_repair_batch(np.zeros((0, 40)), l, u, ints)
    assert out['status'].shape == (0,) and out['x'].shape == (0, 40)
    bad_x = X[:1].copy(); bad_x[0, 3] = np.nan
    bad_l = l.copy(); bad_l[2] = -np.inf
    bad_u = u.copy(); bad_u[2] = np.nan
    for badkw in (dict(integer_indices=[0, 40]), dict(integer_indices=[-1]), dict(integer_indices=[1, 1]), dict(tol=-1.0),
                  dict(max_steps=-1), dict(x=bad_x), dict(l=bad_l), dict(u=bad_u)):
        with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL'):
            p.weighted_repair_batch(**dict(dict(x=X[:1], l=l, u=u, integer_indices=ints), **badkw))
    p.close()   # (MIPX_ETOOBIG cannot be reached from here: no problem above 1024 rows or columns can be made)


@gpu
def test_stand_alone_use_on_a_model(gpu_ctx):
    A, b, c, l, u, ints, X, _, _, _, _, _ = ref.case('mixed-40x20')
    X = X[:9]
    want = ref.weighted_repair(A, b, c, l, u, ints, X)
    mdl = MILPInstance(A=A.copy(), b=b.copy(), c=c.copy(), l=l.copy(), u=u.copy(), sense=['Min', '>='], integerIndices=list(ints),
                       numVars=len(c))
    Xo, obj, status, counts = weighted_repair(mdl, X)
    assert_same(dict(x=Xo, obj=obj, status=status, counts=counts), want)
    one = weighted_repair(mdl, X[1], max_steps=2)
    assert one[0].shape == (1, 40) and one[2][0] in (ref.FEASIBLE, ref.CAPPED) and one[3].sum() <= 2


# ---- the search -------------------------------------------------------------------------------------------------
def arrays(family, seed):
    return random_dense_milp_arrays(40, 20, seed=seed) if family == 'packing' else mixed(20, 10, 5, seed)


def as_model(A, b, c, l, u, ints):
    return MILPInstance(A=A, b=b, c=c, l=l, u=u, sense=['Min', '>='], integerIndices=ints, numVars=len(c))


@functools.lru_cache(maxsize=None)
def highs_optimum(family, seed):
    A, b, c, l, u, ints = arrays(family, seed)
    h = milp(c, constraints=LinearConstraint(A, lb=b, ub=np.inf), bounds=Bounds(l, u), integrality=np.ones(len(c)),
             options={'mip_rel_gap': 0.0})
    assert h.status == 0
    return float(h.fun)


def search(family, seed, Node=PseudoCostBranchNode, frontier_batch=64, **kw):
    bb = BranchAndBound(as_model(*arrays(family, seed)), Node, pseudo_costs={}, gomory_cuts=False, mip_gap=0.0,
                        frontier_batch=frontier_batch, **kw)
    bb.solve()
    return bb


@functools.lru_cache(maxsize=None)
def plain(family, seed):
    bb = search(family, seed)
    return bb.status, float(bb.objective_value), int(bb.evaluated_nodes)


def close(a, b):
    return abs(a - b) <= 1e-6 * max(1.0, abs(b))


def assert_optimal(bb, family, seed, what=''):
    status, value, nodes = plain(family, seed)
    print(what, family, seed, bb.status, bb.objective_value, value, highs_optimum(family, seed), 'nodes', bb.evaluated_nodes, 'plain', nodes,
          bb.weighted_repair_stats, bb.heuristic_stats)
    assert status == 'optimal' and bb.status == status, (what, seed, bb.status)
    assert close(bb.objective_value, value) and close(bb.objective_value, highs_optimum(family, seed))
    rs = bb.root_node.lp._engine_form()
    l, u = bb.root_node.lp._bounds()
    heur.certify(rs.A, rs.b, rs.c, l, u, sorted(bb.model.integerIndices), np.asarray(bb.solution), bb.objective_value, tol=1e-6,
                 int_tol=1e-4, obj_tol=1e-6)


def assert_counters(bb):
    st, hs = bb.weighted_repair_stats, bb.heuristic_stats
    assert list(st) == list(_ffi.WREPAIR_STATS_KEYS)
    assert st['points'] == hs['stuck'] + hs['capped']   # (it runs on the points the rounding did not end feasible on, on all of them)
    assert st['points'] == st['feasible'] + st['capped']   # (the stats add up: there is no third way to end)
    assert st['moves'] >= 0 and st['bumps'] >= 0 and st['reserved6'] == 0
    assert st['feasible'] >= st['incumbents'] and hs['incumbents'] >= st['incumbents']
    assert (st['kernel_us'] > 0) == (hs['points'] > 0)


@functools.lru_cache(maxsize=None)
def searched(family, seed):
    return search(family, seed, primal_heuristic=True, weighted_repair=True)


@gpu
@pytest.mark.parametrize('family,seed', [('mixed', 0), ('mixed', 1), ('mixed', 2), ('mixed', 3), ('packing', 0), ('packing', 1)])
def test_search_with_the_weighted_repair_finds_the_same_optimum(family, seed):
    bb = searched(family, seed)
    assert_optimal(bb, family, seed)
    assert_counters(bb)
    assert search(family, seed, primal_heuristic=True).weighted_repair_stats is None


@gpu
def test_an_incumbent_comes_from_a_weighted_point_on_the_mixed_family():
    """Summed over the four seeds: at least one incumbent is installed from a weighted point, or the heuristic's own
    counters show that its rounding left nothing to repair."""
    total = {k: sum(searched('mixed', seed).weighted_repair_stats[k] for seed in range(4)) for k in _ffi.WREPAIR_STATS_KEYS}
    left = sum(searched('mixed', seed).heuristic_stats['stuck'] + searched('mixed', seed).heuristic_stats['capped'] for seed in range(4))
    print(total, left, [searched('mixed', seed).weighted_repair_stats['incumbents'] for seed in range(4)])
    assert total['incumbents'] >= 1 or left == 0
    assert total['points'] == left


COMBINATIONS = [('propagate', PseudoCostBranchNode, dict(propagate=True)),
                ('reduced cost', PseudoCostBranchNode, dict(reduced_cost=True)),
                ('objective step', PseudoCostBranchNode, dict(objective_step=True)),
                ('local search', PseudoCostBranchNode, dict(local_search=True)),
                ('host spill, small pool', PseudoCostBranchNode, dict(host_spill=1 << 24, frontier_batch=16, pool_capacity=600)),
                ('no anchor', PseudoCostBranchNode, dict(anchor=False)),
                ('plunge of 8', PseudoCostBranchNode, dict(dive=8)),
                ('most fractional', BaseNode, dict()),
                ('all of them', PseudoCostBranchNode, dict(propagate=True, reduced_cost=True, objective_step=True, local_search=True)),
                ('nine steps', PseudoCostBranchNode, dict(weighted_repair=9))]


@gpu
@pytest.mark.parametrize('family,seed', [('packing', 1), ('mixed', 1)])
@pytest.mark.parametrize('what,Node,kw', COMBINATIONS, ids=[c[0] for c in COMBINATIONS])
def test_the_same_optimum_beside_the_other_options(what, Node, kw, family, seed):
    kw = dict(dict(primal_heuristic=True, weighted_repair=True), **kw)
    bb = search(family, seed, Node, **kw)
    assert_optimal(bb, family, seed, what)
    assert_counters(bb)
    if 'local_search' in kw:   # (the pair search runs on the lifted weighted points too)
        assert bb.local_search_stats['points'] == bb.heuristic_stats['feasible'] + bb.weighted_repair_stats['feasible']
    if what == 'nine steps':
        st = bb.weighted_repair_stats
        assert st['moves'] + st['bumps'] <= 9 * st['points']


@gpu
@pytest.mark.parametrize('family,seed', [('packing', 0), ('mixed', 1)])
def test_restart_inherits_the_option(family, seed):
    first = search(family, seed, tree_record=True, primal_heuristic=True, weighted_repair=True)
    assert first.status == 'optimal'
    A, b, c, l, u, ints = arrays(family, seed)
    b2 = b.copy()
    b2[:10] += np.random.default_rng(5).integers(-3, 4, 10)
    again = first.restart(CyLPArray(b2))
    assert again._weighted_repair is True and again._primal_heuristic is True
    again.solve()
    h = milp(c, constraints=LinearConstraint(A, lb=b2, ub=np.inf), bounds=Bounds(l, u), integrality=np.ones(len(c)),
             options={'mip_rel_gap': 0.0})
    print(family, again.status, again.objective_value, h.status, h.fun, again.weighted_repair_stats)
    assert h.status == 0 and again.status == 'optimal' and close(again.objective_value, float(h.fun))
    assert_counters(again)
    off = first.restart(CyLPArray(b2), weighted_repair=None)
    off.solve()
    assert off.weighted_repair_stats is None and close(off.objective_value, float(h.fun))


@gpu
def test_refusals_of_the_c_entry(gpu_ctx):
    A, b, c, l, u, ints = arrays('mixed', 1)
    p = _ffi.Problem(gpu_ctx, A, b, c)
    t = _ffi.Tree(p, ints, l, u, max_batch=16, pool_capacity=1 << 14)
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*mipx_tree_set_heuristic first'):   # without the heuristic
        t.set_weighted_repair(True)
    t.set_heuristic(4)
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*max_steps is not negative'):   # a negative cap
        t.set_weighted_repair(-1)
    t.set_weighted_repair(True)
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*not with the weighted row repair'):   # the dive behind it
        t.set_fix_propagate(True)
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*more points than the weighted row repair was set for'):
        t.set_heuristic(8)
    t.set_weighted_repair(0)   # off again: now the dive may come, and then refuses this option in turn
    t.set_fix_propagate(True)
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*not with the fix-and-propagate dive'):
        t.set_weighted_repair(True)
    t.set_fix_propagate(0)
    t.solve(frontier_batch=16, max_steps=2)
    assert not any(t.weighted_repair_stats().values()) and t.heuristic_stats()['points'] > 0
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*before the first step'):   # after a step
        t.set_weighted_repair(True)
    t.close()
    t = _ffi.Tree(p, ints, l, u, max_batch=16, pool_capacity=1 << 14)
    t.set_heuristic(4)
    t.set_weighted_repair(5)
    s = t.solve(mip_gap=0.0, frontier_batch=16)
    st, hs = t.weighted_repair_stats(), t.heuristic_stats()
    assert _ffi.TREE_STATUS[s['status']] == 'optimal' and close(s['primal_bound'], highs_optimum('mixed', 1))
    assert st['points'] == hs['stuck'] + hs['capped'] == st['feasible'] + st['capped'] and st['moves'] + st['bumps'] <= 5 * st['points']
    t.close()
    p.close()
    with pytest.raises(AssertionError, match='weighted_repair cannot be combined with fix_propagate'):
        search('mixed', 1, primal_heuristic=True, weighted_repair=True, fix_propagate=True)


@gpu
@pytest.mark.parametrize('rule,batch', [('pseudo cost', 1), ('most fractional', 64)])
def test_a_tree_that_never_sets_the_option_is_unchanged(rule, batch, gpu_ctx):
    """Two trees on one instance with the heuristic on, the option never set, the trace on, in the two configurations
    whose order is deterministic: the same trace, node for node, and none of the option's eight counters moves."""
    A, b, c, l, u, ints = mixed(40, 20, 10, 1)

    def run():
        p = _ffi.Problem(gpu_ctx, A, b, c)   # (a problem of its own: the anchor a search sets stays on its problem)
        t = _ffi.Tree(p, ints, l, u, branch_rule=rule, max_batch=batch, pool_capacity=1 << 16)
        if batch > 1:
            t.set_anchor_mode(True)
            t.set_dive(True)
        t.set_heuristic(True)
        t.set_trace(True)
        st = t.solve(mip_gap=0.0, frontier_batch=batch, node_limit=3000)
        out = st, t.trace(), t.weighted_repair_stats(), t.heuristic_stats()
        t.close()
        p.close()
        return out

    st1, tr1, w1, hs1 = run()
    st2, tr2, w2, hs2 = run()
    hs1.pop('kernel_us'); hs2.pop('kernel_us')
    print((rule, batch), (st1['evaluated_nodes'], hs1))
    assert st1['status'] == st2['status'] and st1['primal_bound'] == st2['primal_bound'] and st1['evaluated_nodes'] > 100
    for key in ('evaluated_nodes', 'lp_solved', 'pivots', 'created_nodes', 'steps', 'dives'):
        assert st1[key] == st2[key], key
    for key in ('node_id', 'status', 'branch_var'):
        assert np.array_equal(tr1[key], tr2[key]), key
    assert np.array_equal(bits(tr1['objective']), bits(tr2['objective']))
    assert hs1 == hs2 and hs1['stuck'] > 0
    assert list(w1) == list(_ffi.WREPAIR_STATS_KEYS) and len(w1) == 8 and not any(w1.values()) and not any(w2.values())
