"""K4 through the C ABI (mipx_branch_score_batch / _dev) against the oracle and the reference's own
records, and the assumption BranchAndBound(lp_batch=1) rests on: a node LP solved inside a batch gives
the same bits as solved on its own."""
import json
import os

import numpy as np
import pytest

from simple_mip_solver_amd import _ffi
from simple_mip_solver_amd.generators import random_dense_milp_arrays
from simple_mip_solver_amd.utils import tolerance as tol

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
EPS = tol.variable_epsilon


def adversarial_x(rng, B, n):
    """Exact ties, halves, values at and next to variable_epsilon, integers, large magnitudes."""
    base = rng.integers(-5, 6, (B, n)).astype(np.float64)
    picks = np.array([0.0, 0.5, -0.5, EPS, -EPS, 1 - EPS, np.nextafter(EPS, 1), np.nextafter(EPS, 0), 0.25, 0.75,
                      1e-9, 0.5 + 1e-12, 2.5, -2.5, 1e6 + 0.5])
    x = base + picks[rng.integers(0, len(picks), (B, n))]
    x[0] = 0.5            # every candidate ties: the earliest wins
    x[1] = 3.0            # integral
    x[2] = np.arange(n) + EPS   # exactly at the tolerance: integral
    return x


def check(ctx, ints, x, status, oracle, cost_l=None, cost_r=None):
    rule = 0 if cost_l is None else 1
    n = x.shape[1]
    has = None if rule == 0 else np.ones(n, np.uint8)
    got = _ffi.branch_score_batch(ctx, ints, x, status, rule, cost_l, cost_r, has)
    for k in range(x.shape[0]):
        feasible = status[k] in (0, 2)
        if not feasible:
            assert got['branch_idx'][k] == -1 and not got['mip_feasible'][k]
            continue
        assert got['mip_feasible'][k] == oracle.mip_feasible(ints, x[k]), k
        want = oracle.most_fractional(ints, x[k]) if rule == 0 else \
            oracle.best_pseudo_cost(ints, x[k], cost_l, cost_r)
        assert got['branch_idx'][k] == (-1 if want is None else want), (k, x[k][ints])
        assert got['n_unprobed'][k] == 0
    return got


@pytest.mark.parametrize('n,seed', [(7, 0), (64, 1), (200, 2)])
def test_against_oracle_random_and_adversarial(gpu_ctx, oracle, n, seed):
    rng = np.random.default_rng(seed)
    B = 97
    ints = sorted(rng.choice(n, max(1, n * 2 // 3), replace=False).tolist())
    status = rng.choice([0, 0, 0, 2, 1, 3], B).astype(np.int32)
    status[:3] = 0
    for x in (rng.random((B, n)) * 20 - 10, adversarial_x(rng, B, n)):
        check(gpu_ctx, ints, x, status, oracle)
        cl = rng.choice([0.0, 1.0, 2.5], n)
        cr = rng.choice([0.0, 1.0, 2.5], n)
        check(gpu_ctx, ints, x, status, oracle, cl, cr)


def test_unprobed_candidates_and_empty_integer_set(gpu_ctx):
    x = np.array([[0.5, 1.25, 2.0, 3.75]])
    has = np.array([1, 0, 1, 0], np.uint8)
    got = _ffi.branch_score_batch(gpu_ctx, [0, 1, 2, 3], x, np.zeros(1, np.int32), 1, np.ones(4), np.ones(4), has)
    assert got['n_unprobed'][0] == 2 and got['branch_idx'][0] == 0 and not got['mip_feasible'][0]
    none = _ffi.branch_score_batch(gpu_ctx, [], x, np.zeros(1, np.int32))
    assert none['branch_idx'][0] == -1 and none['mip_feasible'][0]


def test_device_pointer_variant(gpu_ctx, oracle):
    rng = np.random.default_rng(5)
    B, n = 33, 40
    ints = np.arange(0, n, 2, dtype=np.int32)
    x = adversarial_x(rng, B, n)
    status = np.zeros(B, np.int32)
    host = _ffi.branch_score_batch(gpu_ctx, ints, x, status)
    bufs = [gpu_ctx.to_device(a) for a in (ints, x, status)]
    outs = [gpu_ctx.alloc(B * 4) for _ in range(3)]
    try:
        _ffi.branch_score_batch_dev(gpu_ctx, n, B, len(ints), *bufs, 0, None, None, None, *outs)
        got = [np.zeros(B, np.int32) for _ in range(3)]
        for a, d in zip(got, outs):
            gpu_ctx.d2h(a, d)
    finally:
        for d in bufs + outs:
            gpu_ctx.free(d)
    assert np.array_equal(got[0], host['branch_idx'])
    assert np.array_equal(got[1].astype(bool), host['mip_feasible'])


def test_reference_records(gpu_ctx):
    """most_fractional_index (BaseNode) and best_index (PseudoCostBranchNode) as the reference computed them."""
    g = json.load(open(os.path.join(HERE, 'golden', 'base_node.json')))
    seen = 0
    for rec in g['nodes']:
        if 'most_fractional_index' not in rec:
            continue
        x = np.array([rec['x']])
        got = _ffi.branch_score_batch(gpu_ctx, rec['integer_indices'], x, np.zeros(1, np.int32))
        want = rec['most_fractional_index']
        assert got['branch_idx'][0] == (-1 if want is None else want), rec['name']
        seen += 1
    for rec in g['pseudo_costs']:
        if 'best_index' not in rec:
            continue
        n = len(rec['x'])
        cl, cr, has = np.zeros(n), np.zeros(n), np.zeros(n, np.uint8)
        for i, e in rec['table'].items():
            cl[int(i)], cr[int(i)], has[int(i)] = e['left']['cost'], e['right']['cost'], 1
        got = _ffi.branch_score_batch(gpu_ctx, rec['integer_indices'], np.array([rec['x']]),
                                      np.zeros(1, np.int32), 1, cl, cr, has)
        assert got['branch_idx'][0] == rec['best_index']
        seen += 1
    assert seen >= 2


@pytest.mark.parametrize('n,m', [(64, 32), (256, 128)])
def test_batched_node_lps_equal_single(gpu_ctx, n, m):
    """Children of the root on its fractional variables, warm-started: one launch of all of them and
    one launch per node give identical results."""
    A, b, c, l, u, ints = random_dense_milp_arrays(n, m, seed=11)
    p = _ffi.Problem(gpu_ctx, A, b, c)
    root = p.solve_batch(l[None], u[None])
    x = root['x'][0]
    frac = [i for i in ints if min(x[i] - np.floor(x[i]), np.ceil(x[i]) - x[i]) > EPS][:32]
    assert frac
    L = np.repeat(l[None], 2 * len(frac), 0)
    U = np.repeat(u[None], 2 * len(frac), 0)
    for k, i in enumerate(frac):
        U[2 * k, i] = np.floor(x[i])
        L[2 * k + 1, i] = np.ceil(x[i])
    V = np.repeat(root['vstat'], len(L), 0)
    together = p.solve_batch(L, U, V)
    for k in range(len(L)):
        alone = p.solve_batch(L[k:k + 1], U[k:k + 1], V[k:k + 1])
        for key in ('status', 'obj', 'x', 'y', 'vstat', 'iters', 'npivots'):
            assert np.array_equal(together[key][k:k + 1], alone[key]), (k, key)
