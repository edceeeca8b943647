"""The fix-and-propagate dive on the GPU (include/mipx_fixprop.h): the kernel against the NumPy restatement
(tests/support/fix_propagate_reference.py) bit for bit on the cases of that module, and the search with the option on
against the search without it and scipy's milp (HiGHS)."""
import functools

import numpy as np
import pytest
from scipy.optimize import Bounds, LinearConstraint, milp

from simple_mip_solver_amd import BaseNode, BranchAndBound, MILPInstance, PseudoCostBranchNode, _ffi
from simple_mip_solver_amd.generators import random_dense_milp_arrays
from simple_mip_solver_amd.lp import CyLPArray
from simple_mip_solver_amd.utils.fix_propagate import fix_and_propagate
from tests.support import fix_propagate_reference as ref
from tests.support import heuristic_reference as heur
from tests.support.propagation_reference import mixed

gpu = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def assert_same(got, want, count=None):
    """Status, both counts, x~ and obj equal bit for bit, on the points whose rounding decisions were all farther than
    1e-9 from flipping (at most 2 % of a case are not: tests/test_fix_propagate_abi.py checks that on the restatement)."""
    w = {k: v[:count] for k, v in want.items()}
    keep = w['margin'] > 1e-9
    print('status', got['status'][:16], w['status'][:16], 'counts', got['counts'][:6].tolist(), w['counts'][:6].tolist(),
          'left out', int((~keep).sum()))
    assert (~keep).sum() <= 0.02 * len(keep)
    assert np.array_equal(got['status'][keep], w['status'][keep]) and np.array_equal(got['counts'][keep], w['counts'][keep])
    assert np.array_equal(bits(got['x'][keep]), bits(w['x'][keep])) and np.array_equal(bits(got['obj'][keep]), bits(w['obj'][keep]))


@gpu
@pytest.mark.parametrize('name', list(ref.CASES))
def test_kernel_equals_the_restatement_bit_for_bit(name, gpu_ctx):
    A, b, c, l, u, ints, X, cutoff, max_tries, skip, want = ref.case(name)
    p = _ffi.Problem(gpu_ctx, A, b, c)
    got = p.fix_propagate_batch(X, l, u, ints, cutoff=cutoff, tol=ref.TOL, max_tries=max_tries, skip=skip)
    one = p.fix_propagate_batch(X[:1], l, u, ints, cutoff=cutoff, tol=ref.TOL, max_tries=max_tries)   # (a batch of 1)
    p.close()
    assert_same(got, want)
    if skip is None or not skip[0]:
        assert_same(one, want, 1)
    for k in np.flatnonzero(got['status'] == ref.FEASIBLE):
        heur.certify(A, b, c, l, u, ints, got['x'][k], got['obj'][k], tol=ref.TOL)
    same = ~np.isin(got['status'], (ref.FEASIBLE, ref.ROWS))
    assert np.array_equal(bits(got['x'][same]), bits(X[same])) and not got['obj'][same].any()


@gpu
def test_kernel_boxes_without_a_point_caps_rounds_and_refusals(gpu_ctx):
    A, b, c, l, u, ints, X, _, _, _, _ = ref.case('mixed-40x20')
    X = X[:12]
    p = _ffi.Problem(gpu_ctx, A, b, c)
    # a cutoff below every point of the box, and one no point reaches with the rows: INFEASIBLE_BOX, the point untouched
    for cutoff in (float(c @ u) - 1.0, float(c @ u) + 0.5):
        want = ref.fix_propagate(A, b, c, l, u, ints, X, cutoff=cutoff)
        assert np.all(want['status'] == ref.INFEASIBLE_BOX)
        got = p.fix_propagate_batch(X, l, u, ints, cutoff=cutoff, tol=ref.TOL)
        assert_same(got, want)
        assert np.array_equal(bits(got['x']), bits(X)) and not got['counts'].any()
    # caps of 0, 1 and 7 tries, one and two rounds per propagation, and a cutoff of -inf (no cutoff row either)
    for kw in (dict(max_tries=0), dict(max_tries=1), dict(max_tries=7), dict(max_rounds=1), dict(max_rounds=2), dict(cutoff=-np.inf),
               dict(tol=1e-7), dict(tol=1e-3)):
        want = ref.fix_propagate(A, b, c, l, u, ints, X, **kw)
        assert_same(p.fix_propagate_batch(X, l, u, ints, **dict(dict(tol=ref.TOL), **kw)), want)
        if kw.get('max_tries', 99) < 8:
            assert np.all(want['status'] == ref.CAPPED) and np.all(want['counts'][:, 1] == kw['max_tries'])
    # fractional bounds are rounded as the heuristic rounds them; integer columns given in another order
    lf, uf = l - 0.75, u - 0.25   # (rounded: 0 and 9)
    want = ref.fix_propagate(A, b, c, lf, uf, ints, np.clip(X, lf, uf))
    assert np.any(want['status'] == ref.FEASIBLE)
    assert_same(p.fix_propagate_batch(np.clip(X, lf, uf), lf, uf, ints[::-1], tol=ref.TOL), want)
    # an upper bound of +inf: the walk over a column's values is ended by the rows or by the cap
    ui = u.copy(); ui[::3] = np.inf
    want = ref.fix_propagate(A, b, c, l, ui, ints, X, max_tries=60)
    assert_same(p.fix_propagate_batch(X, l, ui, ints, tol=ref.TOL, max_tries=60), want)
    # no integer column at all: the clamped point and its rows
    want = ref.fix_propagate(A, b, c, l, u, [], X)
    assert set(want['status']) <= {ref.FEASIBLE, ref.ROWS}
    assert_same(p.fix_propagate_batch(X, l, u, [], tol=ref.TOL), want)
    # an empty batch is no launch; the refusals
    out = p.fix_propagate_batch(np.zeros((0, 40)), l, u, ints)
    assert out['status'].shape == (0,) and out['x'].shape == (0, 40)
    bad_x = X[:1].copy(); bad_x[0, 3] = np.nan
    bad_l = l.copy(); bad_l[2] = -np.inf
    bad_u = u.copy(); bad_u[2] = np.nan
    for badkw in (dict(integer_indices=[0, 40]), dict(integer_indices=[-1]), dict(integer_indices=[1, 1]), dict(tol=-1.0),
                  dict(max_tries=-1), dict(max_rounds=0), dict(cutoff=np.nan), dict(x=bad_x), dict(l=bad_l), dict(u=bad_u)):
        with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL'):
            p.fix_propagate_batch(**dict(dict(x=X[:1], l=l, u=u, integer_indices=ints), **badkw))
    p.close()   # (MIPX_ETOOBIG cannot be reached from here: no problem above 1024 rows or columns can be made)


@gpu
def test_stand_alone_use_on_a_model(gpu_ctx):
    A, b, c, l, u, ints, X, _, _, _, _ = ref.case('mixed-40x20')
    X = X[:9]
    want = ref.fix_propagate(A, b, c, l, u, ints, X, max_tries=256)
    mdl = MILPInstance(A=A.copy(), b=b.copy(), c=c.copy(), l=l.copy(), u=u.copy(), sense=['Min', '>='], integerIndices=list(ints),
                       numVars=len(c))
    Xo, obj, status, counts = fix_and_propagate(mdl, X, tol=ref.TOL)
    assert_same(dict(x=Xo, obj=obj, status=status, counts=counts), want)
    one = fix_and_propagate(mdl, X[1], cutoff=float(np.median(want['obj'])))
    assert one[0].shape == (1, 40) and one[2][0] in (ref.FEASIBLE, ref.STUCK, ref.INFEASIBLE_BOX)


# ---- the search -------------------------------------------------------------------------------------------------
def arrays(family, seed):
    return random_dense_milp_arrays(40, 20, seed=seed) if family == 'packing' else mixed(40, 20, 10, seed)


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
          bb.fix_propagate_stats, bb.heuristic_stats)
    assert status == 'optimal' and bb.status == status, (what, seed, bb.status)
    assert close(bb.objective_value, value) and close(bb.objective_value, highs_optimum(family, seed))
    rs = bb.root_node.lp._engine_form()
    l, u = bb.root_node.lp._bounds()
    heur.certify(rs.A, rs.b, rs.c, l, u, sorted(bb.model.integerIndices), np.asarray(bb.solution), bb.objective_value, tol=1e-6,
                 int_tol=1e-4, obj_tol=1e-6)


def assert_counters(bb):
    st, hs = bb.fix_propagate_stats, bb.heuristic_stats
    assert list(st) == list(_ffi.FIXPROP_STATS_KEYS)
    assert st['points'] == hs['stuck'] + hs['capped']   # (it runs on the points the rounding did not end feasible on, on all of them)
    assert st['points'] >= st['feasible'] + st['stuck'] + st['capped'] and st['tries'] >= st['fixings'] >= 0
    assert st['feasible'] >= st['incumbents'] and hs['incumbents'] >= st['incumbents']
    assert (st['kernel_us'] > 0) == (hs['points'] > 0)


@functools.lru_cache(maxsize=None)
def searched(family, seed):
    return search(family, seed, primal_heuristic=True, fix_propagate=True)


@gpu
@pytest.mark.parametrize('seed', range(4))
@pytest.mark.parametrize('family', ['packing', 'mixed'])
def test_search_with_the_dive_finds_the_same_optimum(family, seed):
    bb = searched(family, seed)
    assert_optimal(bb, family, seed)
    assert_counters(bb)
    assert search(family, seed, primal_heuristic=True).fix_propagate_stats is None


@gpu
def test_an_incumbent_comes_from_a_dive_point_on_the_mixed_family():
    """Summed over the four seeds: the rounding is stuck on points, the dive ends feasible on some of them, and at least
    one of those becomes the incumbent."""
    total = {k: sum(searched('mixed', seed).fix_propagate_stats[k] for seed in range(4)) for k in _ffi.FIXPROP_STATS_KEYS}
    print(total, [searched('mixed', seed).fix_propagate_stats['incumbents'] for seed in range(4)])
    assert total['points'] > 0 and total['feasible'] > 0 and total['incumbents'] >= 1


COMBINATIONS = [('propagate', PseudoCostBranchNode, dict(propagate=True)),
                ('reduced cost', PseudoCostBranchNode, dict(reduced_cost=True)),
                ('objective step', PseudoCostBranchNode, dict(objective_step=True)),
                ('local search', PseudoCostBranchNode, dict(local_search=True)),
                ('host spill, small pool', PseudoCostBranchNode, dict(host_spill=1 << 24, frontier_batch=16, pool_capacity=600)),
                ('plunge of 8', PseudoCostBranchNode, dict(dive=8)),
                ('most fractional', BaseNode, dict()),
                ('all of them', PseudoCostBranchNode, dict(propagate=True, reduced_cost=True, objective_step=True, local_search=True)),
                ('nine tries', PseudoCostBranchNode, dict(fix_propagate=9))]


@gpu
@pytest.mark.parametrize('family,seed', [('packing', 2), ('mixed', 1)])
@pytest.mark.parametrize('what,Node,kw', COMBINATIONS, ids=[c[0] for c in COMBINATIONS])
def test_the_same_optimum_beside_the_other_options(what, Node, kw, family, seed):
    kw = dict(dict(primal_heuristic=True, fix_propagate=True), **kw)
    bb = search(family, seed, Node, **kw)
    assert_optimal(bb, family, seed, what)
    assert_counters(bb)
    if 'local_search' in kw:   # (the pair search runs on the lifted dive points too)
        assert bb.local_search_stats['points'] == bb.heuristic_stats['feasible'] + bb.fix_propagate_stats['feasible']
    if what == 'nine tries':
        st = bb.fix_propagate_stats
        assert st['tries'] <= 9 * st['points'] and (st['capped'] > 0 or st['points'] == 0)


@gpu
@pytest.mark.parametrize('family,seed', [('packing', 0), ('mixed', 1)])
def test_restart_inherits_the_option(family, seed):
    first = search(family, seed, tree_record=True, primal_heuristic=True, fix_propagate=True)
    assert first.status == 'optimal'
    A, b, c, l, u, ints = arrays(family, seed)
    b2 = b.copy()
    b2[:20] += np.random.default_rng(5).integers(-3, 4, 20)
    again = first.restart(CyLPArray(b2))
    assert again._fix_propagate is True and again._primal_heuristic is True
    again.solve()
    h = milp(c, constraints=LinearConstraint(A, lb=b2, ub=np.inf), bounds=Bounds(l, u), integrality=np.ones(len(c)),
             options={'mip_rel_gap': 0.0})
    print(family, again.status, again.objective_value, h.status, h.fun, again.fix_propagate_stats)
    assert h.status == 0 and again.status == 'optimal' and close(again.objective_value, float(h.fun))
    assert_counters(again)
    off = first.restart(CyLPArray(b2), fix_propagate=None)
    off.solve()
    assert off.fix_propagate_stats is None and close(off.objective_value, float(h.fun))


@gpu
def test_refusals_of_the_c_entry_in_either_order(gpu_ctx):
    A, b, c, l, u, ints = arrays('mixed', 1)
    p = _ffi.Problem(gpu_ctx, A, b, c)
    t = _ffi.Tree(p, ints, l, u, max_batch=16, pool_capacity=1 << 14)
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*mipx_tree_set_heuristic first'):
        t.set_fix_propagate(True)
    t.set_heuristic(4)
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*max_rounds is positive and max_tries is not negative'):
        t.set_fix_propagate(-1)
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*max_rounds is positive'):
        t.set_fix_propagate(True, max_rounds=0)
    t.set_fix_propagate(True)
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*more points than the fix-and-propagate dive was set for'):
        t.set_heuristic(8)
    comm = _ffi.Comm(gpu_ctx, 0, 1, allgather=lambda buf: [buf], send=lambda peer, d: None, recv=lambda peer, k: b'')
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*not with the primal heuristic'):   # (the dive sits on the heuristic)
        t.set_comm(comm, 3)
    t.set_fix_propagate(0)    # off again: the heuristic alone
    t.solve(frontier_batch=16, max_steps=2)
    assert not any(t.fix_propagate_stats().values()) and t.heuristic_stats()['points'] > 0
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*before the first step'):
        t.set_fix_propagate(True)
    t.close()
    # the other order: a tree with a communicator, and one with cut rounds, refuse the heuristic, and so the dive
    t = _ffi.Tree(p, ints, l, u, max_batch=16, pool_capacity=1 << 14)
    t.set_comm(comm, 3)
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*not with a communicator'):
        t.set_heuristic(4)
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*mipx_tree_set_heuristic first'):
        t.set_fix_propagate(True)
    t.set_comm(None)
    t.close()
    comm.close()
    A2, b2, c2, l2, u2, ints2 = random_dense_milp_arrays(20, 10, seed=3)
    p2 = _ffi.Problem(gpu_ctx, A2, b2, c2)
    t = _ffi.Tree(p2, ints2, l2, u2, max_batch=4, pool_capacity=1 << 12, cut_params={})
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*not with cut rounds'):
        t.set_heuristic(4)
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*mipx_tree_set_heuristic first'):
        t.set_fix_propagate(True)
    t.close()
    p2.close()
    t = _ffi.Tree(p, ints, l, u, max_batch=16, pool_capacity=1 << 14)
    t.set_heuristic(4)
    t.set_fix_propagate(5, max_rounds=2)
    s = t.solve(mip_gap=0.0, frontier_batch=16)
    st = t.fix_propagate_stats()
    assert _ffi.TREE_STATUS[s['status']] == 'optimal' and close(s['primal_bound'], highs_optimum('mixed', 1))
    assert st['points'] == t.heuristic_stats()['stuck'] + t.heuristic_stats()['capped'] and st['tries'] <= 5 * st['points']
    t.close()
    p.close()


# evaluated nodes and the heuristic's counters (without its kernel time) of the two fixed searches below on the commit
# before this option existed, measured there with this test's own code
PARENT = {('pseudo cost', 1): (869, dict(points=867, feasible=678, stuck=189, capped=0, repair_moves=753, lift_moves=120, incumbents=3)),
          ('most fractional', 64): (2131, dict(points=746, feasible=479, stuck=267, capped=0, repair_moves=794, lift_moves=83, incumbents=4))}


@gpu
@pytest.mark.parametrize('rule,batch', [('pseudo cost', 1), ('most fractional', 64)])
def test_a_tree_that_never_sets_the_option_is_unchanged(rule, batch, gpu_ctx):
    """Two trees on one instance with the heuristic on, the dive never set, the trace on: the same trace, node for node,
    none of the dive's eight counters moves, and the node count and the heuristic's counters are the parent commit's."""
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
        out = st, t.trace(), t.fix_propagate_stats(), t.heuristic_stats()
        t.close()
        p.close()
        return out

    st1, tr1, f1, hs1 = run()
    st2, tr2, f2, hs2 = run()
    hs1.pop('kernel_us'); hs2.pop('kernel_us')
    print((rule, batch), (st1['evaluated_nodes'], hs1))
    assert st1['status'] == st2['status'] and st1['primal_bound'] == st2['primal_bound'] and st1['evaluated_nodes'] > 100
    for key in ('evaluated_nodes', 'lp_solved', 'pivots', 'created_nodes', 'steps', 'dives'):
        assert st1[key] == st2[key], key
    for key in ('node_id', 'status', 'branch_var'):
        assert np.array_equal(tr1[key], tr2[key]), key
    assert np.array_equal(bits(tr1['objective']), bits(tr2['objective']))
    assert hs1 == hs2 and hs1['stuck'] > 0
    assert list(f1) == list(_ffi.FIXPROP_STATS_KEYS) and len(f1) == 8 and not any(f1.values()) and not any(f2.values())
    assert (st1['evaluated_nodes'], hs1) == PARENT[(rule, batch)]
