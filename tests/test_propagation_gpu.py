"""The bound propagation on the GPU (include/mipx_prop.h): the kernel against the NumPy restatement
(tests/support/propagation_reference.py) bit for bit, and the search with the option on against the search without
it and scipy's milp (HiGHS)."""
import functools
import json
import os

import numpy as np
import pytest
from scipy.optimize import Bounds, LinearConstraint, milp

from simple_mip_solver_amd import (BaseNode, BranchAndBound, MILPInstance,
                                   PseudoCostBranchDepthFirstSearchNode, PseudoCostBranchNode, _ffi)
from simple_mip_solver_amd.generators import random_dense_milp_arrays
from simple_mip_solver_amd.utils.bound_propagation import propagate_bounds
from tests.support import propagation_reference as ref
from tests.support.heuristic_reference import certify

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
INF = float('inf')
BATCHES = [1, 3, 65]
KEYS = ('status', 'changed', 'rounds')


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def case(n, m):
    """One instance per shape, its 65 boxes and the finite cutoff of the shape (computed once)."""
    A, b, c, l, u, ints = random_dense_milp_arrays(n, m, seed=0)
    L, U = ref.boxes(A, b, l, u)
    return frozen(A, b, c, L, U) + (ints, ref.cutoff_for(c, U))


@functools.lru_cache(maxsize=None)
def want(n, m, cut):
    """What the restatement makes of the shape's boxes, without and with the cutoff (computed once)."""
    A, b, c, L, U, ints, cutoff = case(n, m)
    out = ref.propagate(A, b, c, L, U, ints, cutoff=cutoff if cut else INF)
    frozen(*out.values())
    return out


def assert_same(got, exp, count=None):
    sl = slice(0, count)
    for key in KEYS:
        print(key, got[key][:16], exp[key][sl][:16])
        assert np.array_equal(got[key], exp[key][sl]), key
    assert np.array_equal(bits(got['l']), bits(exp['l'][sl])) and np.array_equal(bits(got['u']), bits(exp['u'][sl]))


@pytest.mark.parametrize('cut', [False, True], ids=['no cutoff', 'cutoff'])
@pytest.mark.parametrize('batch', BATCHES)
@pytest.mark.parametrize('n,m', ref.SHAPES)
def test_kernel_equals_the_restatement_bit_for_bit(n, m, batch, cut, gpu_ctx):
    A, b, c, L, U, ints, cutoff = case(n, m)
    exp = want(n, m, cut)
    p = _ffi.Problem(gpu_ctx, A, b, c)
    got = p.propagate_batch(L[:batch], U[:batch], ints, cutoff=cutoff if cut else None)
    p.close()
    assert_same(got, exp, batch)
    inf = got['status'] == ref.INFEASIBLE   # (infeasible nodes come back untouched)
    assert np.array_equal(bits(got['l'][inf]), bits(L[:batch][inf])) and np.array_equal(bits(got['u'][inf]), bits(U[:batch][inf]))


@pytest.mark.parametrize('seed', range(4))
def test_kernel_on_the_mixed_family(seed, gpu_ctx):
    """Packing and covering rows: propagation runs for several rounds, and a cap of 2 stops some boxes early."""
    A, b, c, l, u, ints = ref.mixed(20, 10, 5, seed)
    L, U = ref.boxes(A, b, l, u, seed=seed)
    p = _ffi.Problem(gpu_ctx, A, b, c)
    for rounds, cutoff in ((50, None), (8, None), (2, None), (8, ref.cutoff_for(c, U))):
        exp = ref.propagate(A, b, c, L, U, ints, cutoff=INF if cutoff is None else cutoff, max_rounds=rounds)
        assert_same(p.propagate_batch(L, U, ints, cutoff=cutoff, max_rounds=rounds), exp)
        assert cutoff is not None or exp['rounds'].max() >= min(rounds, 3)
    p.close()


def test_kernel_with_continuous_columns(gpu_ctx):
    """A / 7 and half of the columns continuous: the same bounds bit for bit (they are integers, and no rounding
    decision is within 1e-9 of flipping: tests/test_propagation_abi.py), the continuous columns as they went in."""
    A, b, c, l, u, ints = ref.half_continuous()
    L, U = ref.boxes(A, b, l, u)
    exp = ref.propagate(A, b, c, L, U, ints)
    assert exp['margin'] >= 1e-9
    p = _ffi.Problem(gpu_ctx, A, b, c)
    got = p.propagate_batch(L, U, ints)
    p.close()
    assert_same(got, exp)
    cont = np.setdiff1d(np.arange(A.shape[1]), ints)
    assert np.array_equal(bits(got['l'][:, cont]), bits(L[:, cont])) and np.array_equal(bits(got['u'][:, cont]), bits(U[:, cont]))


def test_kernel_edges(gpu_ctx):
    # x0 + x1 + x2 >= 4 and x0 - x2 >= -1
    A = np.array([[1.0, 1.0, 1.0], [1.0, 0.0, -1.0]]); b = np.array([4.0, -1.0]); c = np.array([1.0, 2.0, 3.0])
    p = _ffi.Problem(gpu_ctx, A, b, c)
    ints = [0, 1, 2]
    boxes = [([0, 0, 0], [2, INF, 1]),       # one infinite term in row 0: only x1 gets a candidate there (ninf = 1)
             ([0, 0, 0], [INF, INF, 1]),     # two infinite terms: row 0 says nothing; row 1 (ninf = 1) bounds x0 from below
             ([0, 0, 0], [INF, INF, INF]),   # row 0 all infinite
             ([1, 2, 1], [1, 2, 1]),         # a point that satisfies the rows
             ([1, 1, 1], [1, 1, 1]),         # a point that does not
             ([0, 0, 3], [1, 5, 4])]         # row 1 cannot hold: infeasible, returned untouched
    L = np.array([bx[0] for bx in boxes], dtype=np.float64); U = np.array([bx[1] for bx in boxes], dtype=np.float64)
    for rounds, cutoff in ((8, None), (1, None), (8, 9.0), (8, 3.0)):
        exp = ref.propagate(A, b, c, L, U, ints, cutoff=INF if cutoff is None else cutoff, max_rounds=rounds)
        got = p.propagate_batch(L, U, ints, cutoff=cutoff, max_rounds=rounds)
        assert_same(got, exp)
        if cutoff is None:
            assert list(got['status'][2:]) == [ref.UNCHANGED, ref.UNCHANGED, ref.INFEASIBLE, ref.INFEASIBLE]
            assert got['status'][0] == ref.TIGHTENED and got['l'][0][1] == 1.0 and got['u'][0][1] == INF
        if rounds == 1:
            assert np.all(got['rounds'] == 1)
        inf = got['status'] == ref.INFEASIBLE
        assert np.array_equal(bits(got['l'][inf]), bits(L[inf])) and np.array_equal(bits(got['u'][inf]), bits(U[inf]))
    assert np.all(p.propagate_batch(L, U, ints, cutoff=3.0)['status'][[0, 1, 2, 3]] == ref.INFEASIBLE)   # (c . x >= 4 on the rows)
    # only integer columns are tightened; an empty batch is no launch
    got = p.propagate_batch(L, U, [0])
    assert np.array_equal(bits(got['l'][:, 1:]), bits(L[:, 1:])) and np.array_equal(bits(got['u'][:, 1:]), bits(U[:, 1:]))
    assert p.propagate_batch(np.zeros((0, 3)), np.zeros((0, 3)), ints)['status'].shape == (0,)
    # the refusals
    for bad in (dict(integer_indices=[0, 3]), dict(integer_indices=[1, 1]), dict(tol=-1.0), dict(max_rounds=0),
                dict(cutoff=float('nan')), dict(l=np.full((1, 3), -INF)), dict(u=np.full((1, 3), float('nan')))):
        kw = dict(dict(l=L[:1], u=U[:1], integer_indices=ints), **bad)
        with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL'):
            p.propagate_batch(**kw)
    p.close()
    # above 1024 rows or columns: no problem can be created to hand to the entry (its own MIPX_ETOOBIG check is
    # behind that one), 1024 columns are taken
    with pytest.raises(_ffi.MipxError, match='MIPX_ETOOBIG'):
        _ffi.Problem(gpu_ctx, np.ones((2, 1025)), np.ones(2), np.ones(1025))
    with pytest.raises(_ffi.MipxError, match='MIPX_ETOOBIG'):
        _ffi.Problem(gpu_ctx, np.ones((1025, 2)), np.ones(1025), np.ones(2))
    Aw, bw, cw = np.ones((2, 1024)), np.array([1024.0, 3.0]), np.ones(1024)
    wide = _ffi.Problem(gpu_ctx, Aw, bw, cw)
    for cutoff in (None, 1000.0):   # (every column must be 1: 1024 bounds change; with the cutoff there is no point)
        exp = ref.propagate(Aw, bw, cw, np.zeros((1, 1024)), np.ones((1, 1024)), np.arange(1024), cutoff=INF if cutoff is None else cutoff)
        assert (exp['status'][0], exp['changed'][0]) == (ref.TIGHTENED if cutoff is None else ref.INFEASIBLE, 1024)
        assert_same(wide.propagate_batch(np.zeros((1, 1024)), np.ones((1, 1024)), np.arange(1024), cutoff=cutoff), exp)
    wide.close()


def test_example_models_keep_their_optimum_inside_the_box():
    """The 64 example models: the root box propagated with the known optimum as the cutoff still holds a point of
    that value (scipy's milp over the propagated box finds it)."""
    table = json.load(open(os.path.join(HERE, 'golden', 'example_models_optima.json')))['models']
    assert len(table) == 64
    tightened = 0
    for f, rec in sorted(table.items()):
        mdl = MILPInstance(file_name=os.path.join(HERE, 'golden', 'example_models', f))
        rs = mdl.lp._engine_form()
        l, u = mdl.lp._bounds()
        opt = rec['milp_opt']
        lo, up, status, changed, rounds = propagate_bounds(mdl, l, u, cutoff=opt + 1e-6 * max(1.0, abs(opt)))
        assert lo.shape == (1, len(l)) and status[0] in (ref.UNCHANGED, ref.TIGHTENED), f
        assert np.all(lo[0] >= l) and np.all(up[0] <= u) and np.all(lo[0] <= up[0]), f
        tightened += int(status[0] == ref.TIGHTENED)
        integrality = np.zeros(len(l)); integrality[sorted(mdl.integerIndices)] = 1
        h = milp(rs.c, constraints=LinearConstraint(rs.A, lb=rs.b, ub=np.inf), bounds=Bounds(lo[0], up[0]),
                 integrality=integrality, options={'mip_rel_gap': 0.0})
        assert h.status == 0 and close(float(h.fun), opt), (f, h.status, h.fun, opt)
    assert tightened >= 1


# ---- the search -------------------------------------------------------------------------------------------------
def arrays(family, seed):
    return random_dense_milp_arrays(40, 20, seed=seed) if family == 'packing' else ref.mixed(20, 10, 5, seed)


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
    return bb.status, float(bb.objective_value)


def close(a, b):
    """tests/test_engine_vs_highs_gpu.py's comparison of two optima: 1e-6 relative."""
    return abs(a - b) <= 1e-6 * max(1.0, abs(b))


def certified(bb):
    """bb.solution satisfies rows, bounds and integrality of the root problem, and c . x is bb.objective_value (rows
    and objective to 1e-6, integrality to 1e-4, the figures of tests/test_engine_vs_highs_gpu.py's comparison)."""
    rs = bb.root_node.lp._engine_form()
    l, u = bb.root_node.lp._bounds()
    certify(rs.A, rs.b, rs.c, l, u, sorted(bb.model.integerIndices), np.asarray(bb.solution), bb.objective_value, tol=1e-6,
            int_tol=1e-4, obj_tol=1e-6)
    return True


def assert_optimal(bb, family, seed, what=''):
    status, value = plain(family, seed)
    print(what, family, seed, bb.status, bb.objective_value, value, highs_optimum(family, seed), bb.propagation_stats)
    assert status == 'optimal' and bb.status == status, (what, seed, bb.status)
    assert close(bb.objective_value, value) and close(bb.objective_value, highs_optimum(family, seed)), \
        (what, seed, bb.objective_value, value, highs_optimum(family, seed))
    assert certified(bb)


@functools.lru_cache(maxsize=None)
def propagated(family, seed):
    return search(family, seed, propagate=True)


@pytest.mark.parametrize('seed', range(4))
@pytest.mark.parametrize('family', ['packing', 'mixed'])
def test_search_with_propagation_finds_the_same_optimum(family, seed):
    bb = propagated(family, seed)
    assert_optimal(bb, family, seed)
    st = bb.propagation_stats
    assert list(st) == list(_ffi.PROP_STATS_KEYS)
    assert st['tightened'] > 0 and st['bounds_changed'] >= st['tightened'] and st['rounds'] >= st['nodes'] > 0
    assert st['nodes'] >= st['tightened'] + st['infeasible'] and st['reserved'] == 0 and st['kernel_us'] > 0
    assert search(family, seed).propagation_stats is None


def test_a_node_is_proven_infeasible_on_the_mixed_family():
    found = [propagated('mixed', seed).propagation_stats['infeasible'] for seed in range(4)]
    print(found)
    assert sum(found) >= 1


COMBINATIONS = [('host spill, small pool', PseudoCostBranchNode, dict(host_spill=1 << 24, frontier_batch=16, pool_capacity=600)),
                ('plunge of 8', PseudoCostBranchNode, dict(dive=8)),
                ('no anchor', PseudoCostBranchNode, dict(anchor=False)),
                ('depth first', PseudoCostBranchDepthFirstSearchNode, dict()),
                ('most fractional', BaseNode, dict()),
                ('one node per step', PseudoCostBranchNode, dict(frontier_batch=1)),
                ('primal heuristic', PseudoCostBranchNode, dict(primal_heuristic=True)),
                ('two rounds', PseudoCostBranchNode, dict(propagate=2))]


@pytest.mark.parametrize('family,seed', [('packing', 2), ('mixed', 1)])
@pytest.mark.parametrize('what,Node,kw', COMBINATIONS, ids=[c[0] for c in COMBINATIONS])
def test_the_same_optimum_beside_the_other_options(what, Node, kw, family, seed):
    kw = dict(dict(propagate=True), **kw)
    bb = search(family, seed, Node, **kw)
    assert_optimal(bb, family, seed, what)
    assert bb.propagation_stats['tightened'] > 0
    if 'host_spill' in kw:
        assert bb.spill_stats is not None
    if 'primal_heuristic' in kw:
        assert bb.heuristic_stats['incumbents'] >= 1
    if what == 'two rounds':
        assert bb.propagation_stats['rounds'] <= 2 * bb.propagation_stats['nodes']


def test_without_the_cutoff_through_the_c_entry(gpu_ctx):
    A, b, c, l, u, ints = ref.mixed(20, 10, 5, 1)
    p = _ffi.Problem(gpu_ctx, A, b, c)
    t = _ffi.Tree(p, ints, l, u, branch_rule='pseudo cost', max_batch=64, pool_capacity=1 << 14)
    t.set_anchor_mode(True)
    t.set_dive(True)
    t.set_propagation(8, use_cutoff=False)
    st = t.solve(mip_gap=0.0, frontier_batch=64)
    stats, x = t.propagation_stats(), t.solution()
    t.close()
    p.close()
    assert st['status'] == 1 and close(st['primal_bound'], highs_optimum('mixed', 1))
    certify(A, b, c, l, u, ints, x, st['primal_bound'], tol=1e-6, int_tol=1e-4, obj_tol=1e-6)
    assert stats['nodes'] > 0 and stats['tightened'] > 0


def test_engine_refusals(gpu_ctx):
    A, b, c, l, u, ints = random_dense_milp_arrays(20, 10, seed=3)
    p = _ffi.Problem(gpu_ctx, A, b, c)
    t = _ffi.Tree(p, ints, l, u, max_batch=4, pool_capacity=1 << 12, cut_params={})
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*not with cut rounds'):
        t.set_propagation(True)
    t.close()
    t = _ffi.Tree(p, ints, l, u, max_batch=4, pool_capacity=1 << 12)
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*max_rounds is positive'):
        t.set_propagation(0)
    t.set_propagation(True)
    comm = _ffi.Comm(gpu_ctx, 0, 1, allgather=lambda buf: [buf], send=lambda peer, d: None, recv=lambda peer, k: b'')
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*not with the bound propagation'):
        t.set_comm(comm, 3)
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*not with the bound propagation'):
        t.set_tree_record(True)
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*not with the bound propagation'):
        t.set_dual_record(1 << 20, 10, np.arange(10, dtype=np.int32), np.ones(10))
    t.solve(frontier_batch=4, max_steps=1)
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*before the first step'):
        t.set_propagation(True)
    t.close()
    t = _ffi.Tree(p, ints, l, u, max_batch=4, pool_capacity=1 << 12)
    t.set_comm(comm, 3)
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*not with a communicator'):
        t.set_propagation(True)
    t.set_comm(None)
    t.close()
    t = _ffi.Tree(p, ints, l, u, max_batch=4, pool_capacity=1 << 12)
    t.set_tree_record(True)
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*not with the tree record'):
        t.set_propagation(True)
    t.close()
    t = _ffi.Tree(p, ints, l, u, max_batch=4, pool_capacity=1 << 12)
    t.set_dual_record(1 << 20, 10, np.arange(10, dtype=np.int32), np.ones(10))
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*not with the dual function'):
        t.set_propagation(True)
    t.close()
    comm.close()
    p.close()


@pytest.mark.parametrize('rule,batch', [('pseudo cost', 1), ('most fractional', 64)])
def test_a_tree_that_never_sets_the_option_is_unchanged(rule, batch, gpu_ctx):
    """Two trees on one instance, the option never set, the trace on: the same trace, node for node, and no
    propagation counter moves.  (The two configurations whose node order does not depend on when the host finishes a
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
        out = st, t.trace(), t.propagation_stats()
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
    assert list(h1) == list(_ffi.PROP_STATS_KEYS) and not any(h1.values()) and not any(h2.values())
