"""The dual function of a frontier-engine search (BranchAndBound(frontier_batch=B, dual_function=...),
include/mipx_dualfn.h): the known values of ISE 418 HW 3 problem 1, parity with the Python path's
find_parameterized_dual_bound, validity against HiGHS at other right-hand sides in the batched
configuration, determinism, the byte cap, the host spill and a shape above the register tiles."""
import glob
import os
import re
import warnings

import numpy as np
import pytest
from scipy.optimize import Bounds, LinearConstraint, milp

from simple_mip_solver_amd import BaseNode, BranchAndBound, CyLPArray, MILPInstance, PseudoCostBranchNode, _ffi
from simple_mip_solver_amd.generators import random_dense_milp_arrays
from tests.support.example_models import model, std_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.abspath(__file__))
DBL_MAX = np.finfo(np.float64).max


def generator_model(n, m, seed):
    A, b, c, l, u, ints = random_dense_milp_arrays(n, m, seed=seed)
    return MILPInstance(A=A, b=b, c=c, l=l, u=u, sense=['Min', '>='], integerIndices=ints, numVars=n), (A, b, c, l, u, ints)


def highs(A, b, c, l, u, ints):
    integrality = np.zeros(len(c))
    integrality[ints] = 1
    h = milp(c, constraints=LinearConstraint(A, lb=b, ub=np.inf), bounds=Bounds(l, u), integrality=integrality,
             options={'mip_rel_gap': 0.0, 'time_limit': 60})
    assert h.status in (0, 2), h.message
    return h.fun if h.status == 0 else np.inf


def close(a, b, rel=1e-9):
    return abs(a - b) <= rel * max(1.0, abs(a), abs(b))


def test_known_values_h3p1():
    from math import isclose
    bb = BranchAndBound(model('h3p1'), gomory_cuts=False, frontier_batch=1, dual_function=True)
    bb.solve()
    assert isclose(bb.find_parameterized_dual_bound(CyLPArray([3.5, -3.5])), bb.objective_value, abs_tol=1e-9)
    sol_bound = {0: 0, 1: .5, 2: 1, 3: 2, 4: 2, 5: 2.5}
    for beta in range(6):
        bound = bb.find_parameterized_dual_bound(CyLPArray(np.array([beta, -beta])))
        assert isclose(sol_bound[beta], bound, abs_tol=1e-9), (beta, bound)
    many = bb.find_parameterized_dual_bounds(np.array([[beta, -beta] for beta in range(6)], dtype=float))
    assert np.allclose(many, [sol_bound[beta] for beta in range(6)], rtol=0, atol=1e-9)


def test_small_branch_infeasible_leaves_resolved_once():
    bb = BranchAndBound(std_model('small_branch'), gomory_cuts=False, frontier_batch=1, dual_function=True)
    bb.solve()
    py = BranchAndBound(std_model('small_branch'), gomory_cuts=False)
    py.solve()
    assert bb.find_parameterized_dual_bound(CyLPArray([-2.5, -4.5])) <= -5.99
    st = bb.dual_function_stats
    assert st['infeasible_leaves'] == 5 and st['penalized_resolves'] == 5 and st['leaves_without_term'] == 0
    for rhs in ([3, 3], [1, 1], [-2.5, -4.5]):
        f = bb.find_parameterized_dual_bound(CyLPArray(rhs))
        assert close(f, py.find_parameterized_dual_bound(CyLPArray(rhs))), rhs
    assert bb.dual_function_stats['penalized_resolves'] == 5   # not again


def check_parity(mdl_factory, Node, kwargs, rhs_list, node_limit=float('inf')):
    bb = BranchAndBound(mdl_factory(), Node, frontier_batch=1, dual_function=True, node_limit=node_limit, **kwargs)
    bb.solve()
    py = BranchAndBound(mdl_factory(), Node, node_limit=node_limit, **kwargs)
    py.solve()
    assert bb.evaluated_nodes == py.evaluated_nodes
    got = bb.find_parameterized_dual_bounds(rhs_list)
    for k, rhs in enumerate(rhs_list):
        want = py.find_parameterized_dual_bound(CyLPArray(rhs))
        assert close(got[k], want), (k, got[k], want)
    # the records: the Python tree's solved nodes and their parents, the same duals, t restated in numpy
    recs = bb._native.dual_records()
    solved = {}
    for v in py.tree.nodes.values():
        n = v.attr['node']
        if n.lp._status == 0 and getattr(n.lp, 'nVariables', 0) == py.root_node.lp.nVariables:
            solved[n.idx] = n
    own = recs['status'] == 0
    assert sorted(recs['node'][own].tolist()) == sorted(solved)
    lp0 = py.root_node.lp
    rs = lp0._engine_form()
    pos, plus = lp0._row_index()
    sign = np.where(plus, 1.0, -1.0)
    for r in np.flatnonzero(own):
        n = solved[int(recs['node'][r])]
        lin = n.lineage
        assert recs['parent'][r] == (lin[-2] if len(lin) > 1 else -1)
        y = recs['y'][r]
        if len(set(pos.tolist())) == len(pos):   # one engine row per LP row: the engine duals come back exactly
            assert np.array_equal(y, sign * n.lp._row_duals[pos])
        d = rs.c - rs.A.T @ y
        terms = np.maximum(d, 0) * n.lp.variablesLower + np.minimum(d, 0) * n.lp.variablesUpper
        assert abs(recs['t'][r] - terms.sum()) <= 1e-12 * max(1.0, np.abs(terms).sum())


@pytest.mark.parametrize('Node', [BaseNode, PseudoCostBranchNode])
def test_parity_value_function_fixtures(Node):
    folders = sorted(glob.glob(os.path.join(ROOT, 'golden', 'example_value_functions', 'instance_*')))
    assert len(folders) == 5
    for folder in folders:
        files = glob.glob(os.path.join(folder, 'evaluation_*.mps'))
        rhs = [-MILPInstance(file_name=f).b for f in sorted(files, key=lambda f: int(re.search(r'_(\d+).mps', f).group(1)))]
        assert len(rhs) == 40
        f0 = os.path.join(folder, 'evaluation_0.mps')
        check_parity(lambda: MILPInstance(file_name=f0), Node, dict(pseudo_costs={}, gomory_cuts=False), rhs)


@pytest.mark.parametrize('n,m', [(20, 10), (30, 15), (40, 20)])
@pytest.mark.parametrize('node_limit', [float('inf'), 15])
def test_parity_generator(n, m, node_limit):
    _, (A, b, c, l, u, ints) = generator_model(n, m, 3)
    rng = np.random.default_rng(5)
    rhs = [b + rng.uniform(-2, 2, m) for _ in range(8)] + [b]
    for Node in (BaseNode, PseudoCostBranchNode):
        check_parity(lambda: generator_model(n, m, 3)[0], Node, dict(pseudo_costs={}, gomory_cuts=False), rhs,
                     node_limit=node_limit)


def perturbed(b, rng, K):
    scale = np.maximum(1.0, np.abs(b))
    out = [b - rng.uniform(0, 0.3, len(b)) * scale for _ in range(K // 2)]      # relaxed
    out += [b + rng.uniform(0, 0.05, len(b)) * scale for _ in range(K - K // 2)]  # tightened
    return np.array(out)


@pytest.mark.parametrize('n,m', [(60, 30), (80, 40)])
def test_valid_in_the_batched_configuration(n, m):
    mdl, (A, b, c, l, u, ints) = generator_model(n, m, 1)
    bb = BranchAndBound(mdl, PseudoCostBranchNode, pseudo_costs={}, gomory_cuts=False, frontier_batch=256,
                        dual_function=True, mip_gap=0.0, pool_capacity=1 << 20)
    bb.solve()
    assert bb.status == 'optimal'
    tol = 1e-6 * max(1.0, abs(bb.objective_value))
    fb = bb.find_parameterized_dual_bound(CyLPArray(b))
    assert bb.dual_bound - tol <= fb <= bb.objective_value + tol
    B = perturbed(b, np.random.default_rng(n), 32)
    f = bb.find_parameterized_dual_bounds(B)
    for k in range(len(B)):
        opt = highs(A, B[k], c, l, u, ints)
        assert f[k] <= opt + 1e-6 * max(1.0, abs(opt) if np.isfinite(opt) else 1.0), (k, f[k], opt)
    st = bb.dual_function_stats
    assert st['records'] > 0 and st['dropped'] == 0


def test_determinism_and_traced_records(gpu_ctx):
    A, b, c, l, u, ints = random_dense_milp_arrays(60, 30, seed=2)
    pos, sign = np.arange(30), np.ones(30)
    W = perturbed(b, np.random.default_rng(0), 24)
    runs = []
    for trace in (False, True, False):
        p = _ffi.Problem(gpu_ctx, A, b, c)
        t = _ffi.Tree(p, ints, l, u, branch_rule='pseudo cost', max_batch=64, pool_capacity=1 << 16)
        t.set_anchor_mode(True)
        t.set_dive(4)
        t.set_dual_record(1 << 30, 30, pos, sign)
        if trace:
            t.set_trace(True)
        t.solve(mip_gap=0.0, frontier_batch=64, max_steps=12)
        many = t.dual_function(W, 1e9)
        single = np.array([t.dual_function(W[k], 1e9)[0] for k in range(len(W))])
        assert np.array_equal(many.view(np.int64), single.view(np.int64))
        runs.append((t.dual_records(), many))
        t.close()
        p.close()
    for recs, many in runs[1:]:
        assert np.array_equal(many.view(np.int64), runs[0][1].view(np.int64))
        for key in ('node', 'parent', 'status'):
            assert np.array_equal(recs[key], runs[0][0][key]), key
        assert np.array_equal(recs['t'].view(np.int64), runs[0][0]['t'].view(np.int64))
        assert np.array_equal(recs['y'].view(np.int64), runs[0][0]['y'].view(np.int64))


def test_byte_cap():
    mdl, (A, b, c, l, u, ints) = generator_model(60, 30, 1)
    full = BranchAndBound(mdl, PseudoCostBranchNode, pseudo_costs={}, gomory_cuts=False, frontier_batch=256,
                          dual_function=True)
    full.solve()
    mdl2, _ = generator_model(60, 30, 1)
    capped = BranchAndBound(mdl2, PseudoCostBranchNode, pseudo_costs={}, gomory_cuts=False, frontier_batch=256,
                            dual_function=40 * 8 * 31)
    with pytest.warns(RuntimeWarning, match='dual function store is full'):
        capped.solve()
    assert capped.dual_function_stats['dropped'] > 0
    B = np.vstack([b[None], perturbed(b, np.random.default_rng(9), 16)])
    fc, ff = capped.find_parameterized_dual_bounds(B), full.find_parameterized_dual_bounds(B)
    for k in range(len(B)):
        opt = highs(A, B[k], c, l, u, ints)
        assert fc[k] <= ff[k] and fc[k] <= opt + 1e-6 * max(1.0, abs(opt) if np.isfinite(opt) else 1.0)


def test_host_spill_records_equal_a_large_pool():
    out = []
    for pool, spill in ((1 << 16, None), (3 * 64 * 7 * 2 + 1, 1 << 30)):
        mdl, (A, b, c, l, u, ints) = generator_model(60, 30, 4)
        bb = BranchAndBound(mdl, PseudoCostBranchNode, pseudo_costs={}, gomory_cuts=False, frontier_batch=64,
                            dive=2, pool_capacity=pool, host_spill=spill, dual_function=True)
        bb.solve()
        recs = bb._native.dual_records()
        out.append((recs, bb.find_parameterized_dual_bounds(perturbed(b, np.random.default_rng(1), 16)),
                    bb.spill_stats))
    (r0, f0, _), (r1, f1, sp) = out
    print('spill stats', sp)
    for key in ('node', 'parent', 'status'):
        assert np.array_equal(r0[key], r1[key]), key
    assert np.array_equal(r0['t'].view(np.int64), r1['t'].view(np.int64))
    assert np.array_equal(r0['y'].view(np.int64), r1['y'].view(np.int64))
    assert np.array_equal(f0.view(np.int64), f1.view(np.int64))


def test_above_the_register_tiles():
    """300 x 150 (K1b / K1c write the duals) with a node limit: valid at b, monotone in b, and at a relaxed
    b' <= b below the objective of any point feasible at b (the incumbent, or HiGHS's within a time limit)."""
    mdl, (A, b, c, l, u, ints) = generator_model(300, 150, 0)
    bb = BranchAndBound(mdl, PseudoCostBranchNode, pseudo_costs={}, gomory_cuts=False, frontier_batch=256,
                        dual_function=True, node_limit=5000, pool_capacity=1 << 18)
    bb.solve()
    assert bb.dual_function_stats['records'] > 0
    fb = bb.find_parameterized_dual_bound(CyLPArray(b))
    tol = 1e-6 * max(1.0, abs(fb))
    assert bb.dual_bound - tol <= fb
    if bb.objective_value is not None and bb.objective_value < np.inf:
        assert fb <= bb.objective_value + tol
        x = np.asarray(bb.solution, dtype=np.float64)
    else:
        integrality = np.zeros(len(c))
        integrality[ints] = 1
        h = milp(c, constraints=LinearConstraint(A, lb=b, ub=np.inf), bounds=Bounds(l, u), integrality=integrality,
                 options={'time_limit': 30})
        x = h.x
    rng = np.random.default_rng(3)
    relaxed = np.array([b - rng.uniform(0, 0.5, len(b)) * np.maximum(1.0, np.abs(b)) for _ in range(8)])
    f = bb.find_parameterized_dual_bounds(relaxed)
    assert np.all(f <= fb + tol)
    if x is not None:
        cx = float(c @ x)
        assert np.all(f <= cx + 1e-6 * max(1.0, abs(cx)))


def test_solve_again_continues_recording(gpu_ctx):
    """A search stopped by its step limit and continued: the records grow, the next evaluation sees the new
    leaves, and every value stays below HiGHS's optimum."""
    A, b, c, l, u, ints = random_dense_milp_arrays(40, 20, seed=6)
    p = _ffi.Problem(gpu_ctx, A, b, c)
    t = _ffi.Tree(p, ints, l, u, branch_rule='pseudo cost', max_batch=64, pool_capacity=1 << 16)
    t.set_anchor_mode(True)
    t.set_dive(2)
    t.set_dual_record(1 << 28, 20, np.arange(20), np.ones(20))
    W = perturbed(b, np.random.default_rng(2), 8)
    t.solve(mip_gap=0.0, frontier_batch=64, max_steps=2)
    r1 = t.dual_function_stats()['records']
    f1 = t.dual_function(W, 1e9)
    st = t.solve(mip_gap=0.0, frontier_batch=64)
    assert st['status'] == 1 and t.dual_function_stats()['records'] > r1
    f2 = t.dual_function(W, 1e9)
    for k in range(len(W)):
        opt = highs(A, W[k], c, l, u, ints)
        bound = opt + 1e-6 * max(1.0, abs(opt) if np.isfinite(opt) else 1.0)
        assert f1[k] <= bound and f2[k] <= bound
    tol = 1e-6 * max(1.0, abs(st['primal_bound']))
    assert abs(t.dual_function(b, 1e9)[0] - st['primal_bound']) <= tol
    t.close()
    p.close()
