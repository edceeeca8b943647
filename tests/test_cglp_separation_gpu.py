"""Disjunctive cuts from a recorded tree by batched leaf separation (DisjunctiveSeparator, include/mipx_cglp.h).
The judge is HiGHS, never the engine: the support value of the returned cut on every leaf, and the optimum of
the extended formulation with the same box normalisation, built as a sparse matrix (tests/support/cglp_reference.py).
Margins: validity 1e-7 max(1, |pi0|, |pi|_1), the one test_cut_from_a_batched_tree_is_valid_on_every_leaf uses;
optimality the separator's own stopping slack (its tol on that scale) plus HiGHS's feasibility tolerance (1e-7)
on the same scale -- the two optima are equal by LP duality."""
import json
import os

import numpy as np
import pytest

from simple_mip_solver_amd import BaseNode, BranchAndBound, DisjunctiveSeparator, MILPInstance, PseudoCostBranchNode, _ffi
from simple_mip_solver_amd.generators import random_dense_milp_arrays
from tests.support import cglp_reference as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.abspath(__file__))
N, M, SEED = 40, 20, 3
HIGHS_TOL = 1e-7


def generator_model(n, m, seed):
    A, b, c, l, u, ints = random_dense_milp_arrays(n, m, seed=seed)
    return MILPInstance(A=A, b=b, c=c, l=l, u=u, sense=['Min', '>='], integerIndices=ints, numVars=n)


def scale_of(pi, pi0):
    return max(1.0, abs(pi0), float(np.abs(np.asarray(pi)).sum()))


def childless_not_infeasible(bb):
    rec = bb.tree.rec
    return np.flatnonzero(((rec['flags'] & _ffi.TR_HAS_CHILDREN) == 0) & (rec['lp_status'] != 1))


def grown_tree(**extra):
    """A 40 x 20 search in batches of 64, continued until the tree has 500 not-infeasible childless nodes."""
    bb = BranchAndBound(generator_model(N, M, SEED), PseudoCostBranchNode, pseudo_costs={}, gomory_cuts=False,
                        frontier_batch=64, tree_record=True, mip_gap=0.0, node_limit=1200, **extra)
    bb.solve()
    while len(childless_not_infeasible(bb)) < 500 and bb.status != 'optimal':
        bb.node_limit += 600
        bb.solve()
    return bb


_cache = {}


def big_tree():
    if 'big' not in _cache:
        _cache['big'] = grown_tree()
    return _cache['big']


def check_valid_on_every_leaf(bb, sep, pi, pi0, what):
    """Check 2: h_t(pi) by HiGHS over every not-infeasible childless node's own bounds; returns the worst margin."""
    A, b, _, _, _, _ = random_dense_milp_arrays(N, M, seed=SEED)
    pi = np.asarray(pi, np.float64)
    ids = childless_not_infeasible(bb)
    L, U = bb._native.node_bounds(ids)
    margin = 1e-7 * scale_of(pi, pi0)
    worst, infeasible = np.inf, []
    for k, i in enumerate(ids):
        status, h = ref.support(pi, A, b, L[k], U[k])
        if status == 2:
            infeasible.append(int(i))
            continue
        assert status == 0, (what, i, status)
        worst = min(worst, h - pi0)
    print(what, 'leaves', len(ids), 'HiGHS-infeasible', len(infeasible), 'worst margin', worst, 'allowed', -margin)
    assert sorted(infeasible) == sorted(int(i) for i in sep.dropped_ids), (what, infeasible, sep.dropped_ids)
    assert len(ids) - len(infeasible) == sep.stats['leaves']
    assert worst >= -margin, (what, worst, margin)
    return worst


# ---- 1, 2. beyond the wall; valid on every leaf --------------------------------------------------------
def test_cut_from_a_tree_beyond_the_lp_kernels_columns():
    bb = big_tree()
    ids = childless_not_infeasible(bb)
    assert len(ids) >= 500
    rows, cols = ref.extended_formulation_size(len(ids), N, M)
    print('leaves', len(ids), 'extended formulation', rows, 'x', cols)
    assert cols > 1024 and rows > 1024
    sep = DisjunctiveSeparator(bb, 0)
    assert sorted(sep.leaf_ids) == sorted(ids)
    pi, pi0 = sep.solve()
    print('stats', sep.stats)
    assert pi is not None and sep.stats['converged']
    x_root = np.asarray(bb.root_node.solution, np.float64)
    assert float(np.asarray(pi) @ x_root) < pi0   # the root solution violates the cut
    assert np.all(np.abs(np.asarray(pi)) <= 1.0)
    _cache['big cut'] = (sep, np.asarray(pi).copy(), pi0)


def test_cut_is_valid_on_every_leaf_by_highs():
    bb = big_tree()
    if 'big cut' not in _cache:
        sep = DisjunctiveSeparator(bb, 0)
        pi, pi0 = sep.solve()
        _cache['big cut'] = (sep, np.asarray(pi).copy(), pi0)
    sep, pi, pi0 = _cache['big cut']
    check_valid_on_every_leaf(bb, sep, pi, pi0, 'converged cut')


# ---- 3. optimal, judged by HiGHS -------------------------------------------------------------------------
def highs_optimum(terms, x_star):
    live = [t for t in terms if ref.support(np.zeros(len(x_star)), *t)[0] == 0]   # (an empty term is no term)
    res = ref.extended_formulation(live, x_star)
    assert res.status == 0, res.message
    return float(res.fun), len(live)


def test_optimum_equals_the_extended_formulations():
    """40 x 20, seed 3, frontier_batch=1, node_limit=100: 101 leaves (HiGHS solves their extended formulation,
    4 141 rows x 10 141 columns, to status 0)."""
    A, b, _, _, _, _ = random_dense_milp_arrays(N, M, seed=SEED)
    bb = BranchAndBound(generator_model(N, M, SEED), BaseNode, gomory_cuts=False, frontier_batch=1, tree_record=True,
                        node_limit=100)
    bb.solve()
    tol = 1e-7
    sep = DisjunctiveSeparator(bb, 0, tol=tol)
    assert 50 <= len(sep.leaf_ids) <= 200
    pi, pi0 = sep.solve()
    assert pi is not None and sep.stats['converged']
    x_star = np.asarray(bb.root_node.solution, np.float64)
    L, U = bb._native.node_bounds(sep.leaf_ids)
    want, live = highs_optimum([(A, b, L[k], U[k]) for k in range(len(sep.leaf_ids))], x_star)
    got = float(np.asarray(pi) @ x_star) - pi0
    allowed = (tol + HIGHS_TOL) * scale_of(pi, pi0)
    print('leaves', len(sep.leaf_ids), 'live', live, 'separator', got, 'HiGHS', want, 'difference', got - want, 'allowed', allowed,
          'stats', sep.stats)
    assert live == sep.stats['leaves']
    assert abs(got - want) <= allowed


# ---- 4. same hull, same value ------------------------------------------------------------------------------
def example_models():
    table = json.load(open(os.path.join(ROOT, 'golden', 'example_models_optima.json')))['models']
    return [f for k, f in enumerate(sorted(table)) if not (k % 3 or k == 3)]


@pytest.mark.parametrize('f', example_models())
def test_recorded_tree_and_python_tree_give_the_same_optimum(f):
    m = MILPInstance(file_name=os.path.join(ROOT, 'golden', 'example_models', f))
    py = BranchAndBound(m, node_limit=8, gomory_cuts=False)
    py.solve()
    bb = BranchAndBound(m, node_limit=8, gomory_cuts=False, frontier_batch=1, tree_record=True)
    bb.solve()
    x_star = np.asarray(py.root_node.solution, np.float64)
    terms = []
    for leaf in py.tree.get_leaves(0, keep='not infeasible'):
        A, b = ref.ge_rows(leaf.lp)
        terms.append((A, b, np.asarray(leaf.lp.variablesLower, np.float64), np.asarray(leaf.lp.variablesUpper, np.float64)))
    want, live = highs_optimum(terms, x_star)
    tol = 1e-7
    sep = DisjunctiveSeparator(bb, 0, tol=tol)
    pi, pi0 = sep.solve()
    print(f, 'leaves', len(terms), 'live', live, 'HiGHS', want, 'stats', sep.stats)
    assert sep.stats['leaves'] == live
    if pi is None:   # no cut is violated: the extended formulation says so too
        allowed = (tol + HIGHS_TOL) * max(1.0, sep.R)
        assert want >= -allowed, (want, sep.stats)
        return
    got = float(np.asarray(pi) @ x_star) - pi0
    allowed = (tol + HIGHS_TOL) * scale_of(pi, pi0)
    print('separator', got, 'difference', got - want, 'allowed', allowed)
    assert sep.stats['converged'] and abs(got - want) <= allowed


# ---- 5. always valid -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('max_rounds', [1, 3])
def test_a_stopped_separator_still_returns_a_valid_cut(max_rounds):
    bb = big_tree()
    sep = DisjunctiveSeparator(bb, 0, max_rounds=max_rounds)
    pi, pi0 = sep.solve()
    assert sep.stats['rounds'] == max_rounds and not sep.stats['converged']
    best_pi, best_pi0 = sep.best_cut   # (the best valid cut met, returned only if the root solution violates it)
    if pi is None:
        assert sep.stats['violation'] <= 0
    else:
        assert np.array_equal(np.asarray(pi), best_pi) and pi0 == best_pi0
    check_valid_on_every_leaf(bb, sep, best_pi, best_pi0, f'max_rounds={max_rounds}')


# ---- 6. deterministic ------------------------------------------------------------------------------------------
def test_two_sessions_agree_bit_for_bit():
    bb = big_tree()
    out = []
    for _ in range(2):
        sep = DisjunctiveSeparator(bb, 0)
        pi, pi0 = sep.solve()
        out.append((np.asarray(pi).view(np.int64).copy(), np.float64(pi0).view(np.int64), dict(sep.stats)))
        sep.close()
    assert np.array_equal(out[0][0], out[1][0]) and out[0][1] == out[1][1]
    assert out[0][2] == out[1][2]


# ---- 7. beside the other options ----------------------------------------------------------------------------------
def test_beside_host_spill_dive_and_dual_function():
    extra = dict(host_spill=1 << 30, dive=8, dual_function=True)
    bb = grown_tree(**extra)
    plain = grown_tree(**extra)   # the same search, no session ever opened
    sep = DisjunctiveSeparator(bb, 0)
    pi, pi0 = sep.solve()
    assert pi is not None and sep.stats['converged']
    assert len(sep.leaf_ids) >= 500 and ref.extended_formulation_size(len(sep.leaf_ids), N, M)[1] > 1024
    assert float(np.asarray(pi) @ np.asarray(bb.root_node.solution, np.float64)) < pi0
    check_valid_on_every_leaf(bb, sep, pi, pi0, 'with host_spill, dive=8, dual_function')
    sep.close()
    # the session changed nothing of the search: continue both searches to the same limit
    for run in (bb, plain):
        run.node_limit += 600
        run.solve()
    assert bb.status == plain.status and bb.evaluated_nodes == plain.evaluated_nodes
    assert np.float64(bb.objective_value).view(np.int64) == np.float64(plain.objective_value).view(np.int64)
    assert bb.dual_function_stats['records'] == plain.dual_function_stats['records']


# ---- the session itself ------------------------------------------------------------------------------------------
def test_session_rows_are_the_smallest_margins_in_order():
    """The output block against the full margins of the same evaluation: the rows are the leaves of smallest
    (margin, node id), each with h_t = pi.x_t and x_t inside its leaf's box."""
    bb = big_tree()
    ids = childless_not_infeasible(bb)
    ses = bb._native.support_open(ids)
    rng = np.random.default_rng(0)
    for round_ in range(3):
        pi = rng.uniform(-1, 1, N)
        res = ses.eval(pi, 0.5, tol=1e-6, max_points=16, want_margins=True)
        live = ses.leaves()
        assert res['leaves'] == len(live) == len(res['margins']) and res['not_optimal'] == 0
        order = np.lexsort((live, res['margins']))[:16]
        assert np.array_equal(res['ids'], live[order])
        assert np.array_equal(res['h'] - 0.5, res['margins'][order])
        assert res['min_margin'] == res['margins'].min() and res['min_id'] == live[order[0]]
        assert res['below'] == int((res['margins'] < -1e-6).sum())
        L, U = bb._native.node_bounds(res['ids'])
        assert np.all(res['x'] >= L - 1e-7) and np.all(res['x'] <= U + 1e-7)
        assert np.allclose(res['x'] @ pi, res['h'], rtol=0, atol=1e-9 * max(1.0, float(np.abs(res['h']).max())))
    st = ses.stats()
    assert st['evaluations'] == 3 and st['leaf_lps'] >= 3 * len(live) and st['kernel_ms'] > 0
    assert sorted(np.concatenate([live, ses.leaves(dropped=True)])) == sorted(ids)
    ses.close()


def test_engine_refusals(gpu_ctx):
    A, b, c, l, u, ints = random_dense_milp_arrays(20, 10, seed=3)
    p = _ffi.Problem(gpu_ctx, A, b, c)
    t = _ffi.Tree(p, ints, l, u, max_batch=4, pool_capacity=1 << 12)
    t.solve(frontier_batch=4, max_steps=2)
    with pytest.raises(_ffi.MipxError, match='recording is off'):
        t.support_open([0])
    t.close()
    t = _ffi.Tree(p, ints, l, u, max_batch=4, pool_capacity=1 << 12)
    t.set_tree_record(True)
    t.solve(frontier_batch=4, max_steps=2)
    with pytest.raises(_ffi.MipxError, match='outside the tree'):
        t.support_open([10 ** 6])
    with pytest.raises(_ffi.MipxError, match='given twice'):
        t.support_open([1, 1])
    ses = t.support_open([1, 2])
    with pytest.raises(_ffi.MipxError, match='bad argument'):
        ses.eval(np.zeros(20), 0.0, max_points=0)
    t.close()   # (closes the session with it)
    assert ses._h is None
    lu = u.copy()
    lu[3] = np.inf
    t = _ffi.Tree(p, ints, l, lu, max_batch=4, pool_capacity=1 << 12)
    t.set_tree_record(True)
    t.solve(frontier_batch=4, max_steps=2)
    with pytest.raises(_ffi.MipxError, match='infinite bound'):
        t.support_open([0])
    t.close()
    p.close()
