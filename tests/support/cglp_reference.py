"""HiGHS as the judge of a disjunctive cut (test infrastructure only): the support value of a cut direction on
one term, and the extended formulation of the cut-generating LP with the box normalisation -1 <= pi <= 1, built
as a sparse matrix.  Nothing here uses the engine."""
import numpy as np
from scipy.optimize import linprog
from scipy.sparse import bmat, csr_matrix, eye

COIN = 1e300


def ge_rows(lp):
    """The rows of a DenseLP as A x >= b (a <= side negated, a ranged row entered twice)."""
    A = np.asarray(lp.dense_rows(), np.float64)
    lo, up = np.asarray(lp.constraintsLower, np.float64), np.asarray(lp.constraintsUpper, np.float64)
    has_lo, has_up = lo > -COIN, up < COIN
    return np.vstack([A[has_lo], -A[has_up]]), np.concatenate([lo[has_lo], -up[has_up]])


def support(pi, A, b, lo, up):
    """(status, min pi.x over {A x >= b, lo <= x <= up}) by HiGHS."""
    res = linprog(pi, A_ub=-A, b_ub=-b, bounds=list(zip(lo, up)), method='highs')
    return res.status, (float(res.fun) if res.status == 0 else None)


def extended_formulation_size(T, n, m):
    """(rows, columns) of the reference's cut-generating LP over T terms of m rows and n columns."""
    return T * (n + 1) + 1, n + 1 + T * (m + 2 * n)


def extended_formulation(terms, x_star):
    """min x*.pi - pi0 over the cuts valid for every term (A, b, lo, up) with -1 <= pi <= 1, in the multipliers
    of every term (Farkas): pi = A_t' u_t + w_t - v_t, pi0 <= b_t.u_t + lo_t.w_t - up_t.v_t, u, w, v >= 0.
    Columns [pi | pi0 | u_1 w_1 v_1 | ...].  Returns the linprog result (x[:n] = pi, x[n] = pi0)."""
    n = len(x_star)
    T = len(terms)
    blocks = [[None] * (2 + T) for _ in range(2 * T)]
    for t, (A, b, lo, up) in enumerate(terms):
        m = len(b)
        blocks[2 * t][0] = -eye(n, format='csr')
        blocks[2 * t][2 + t] = csr_matrix(np.hstack([A.T, np.eye(n), -np.eye(n)]))
        blocks[2 * t + 1][1] = csr_matrix(np.array([[1.0]]))                       # pi0 - (b.u + lo.w - up.v) <= 0
        blocks[2 * t + 1][2 + t] = csr_matrix(-np.concatenate([b, lo, -up])[None])
        assert m + 2 * n == blocks[2 * t][2 + t].shape[1]
    M = bmat(blocks, format='csr')
    eq = np.repeat(np.arange(T) * (n + 1), n) + np.tile(np.arange(n), T)
    ub = np.arange(T) * (n + 1) + n
    cost = np.zeros(M.shape[1])
    cost[:n], cost[n] = x_star, -1.0
    bounds = [(-1.0, 1.0)] * n + [(None, None)] + [(0.0, None)] * (M.shape[1] - n - 1)
    return linprog(cost, A_eq=M[eq], b_eq=np.zeros(len(eq)), A_ub=M[ub], b_ub=np.zeros(T), bounds=bounds, method='highs')
