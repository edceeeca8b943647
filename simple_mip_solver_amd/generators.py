"""Synthetic random dense MILPs.

Restates the distribution of the reference's wrapper around grumpy's GenerateRandomMIP
(test_simple_mip_solver/example_models.py:12-25): integer c_j ~ U{1..maxObjCoeff},
A_ij ~ U{1..maxConsCoeff} with probability `density` (else 0),
b_i ~ U{floor(n*density*maxConsCoeff/tightness) .. floor(n*density*maxConsCoeff/1.5)};
problem  max c'x, Ax <= b, 0 <= x <= maxObjCoeff, x integer, handed to the solver as
min -c'x, -Ax >= -b (example_models.py:24-25).  RNG: numpy Generator(PCG64(seed)).
"""
import numpy as np


def random_dense_milp_arrays(num_vars, num_cons, density=1.0, max_obj_coeff=10,
                             max_cons_coeff=10, tightness=2, seed=0):
    """Return (A, b, c, l, u, integer_indices) already in `min c'x, Ax >= b` form."""
    rng = np.random.Generator(np.random.PCG64(seed))
    n, m = int(num_vars), int(num_cons)
    c = rng.integers(1, max_obj_coeff + 1, n).astype(np.float64)
    A = rng.integers(1, max_cons_coeff + 1, (m, n)).astype(np.float64)
    if density < 1.0:
        A *= rng.random((m, n)) < density
    lo = int(n * density * max_cons_coeff / tightness)
    hi = int(n * density * max_cons_coeff / 1.5)
    b = rng.integers(lo, hi + 1, m).astype(np.float64)
    l = np.zeros(n)
    u = np.full(n, float(max_obj_coeff))
    return -A, -b, -c, l, u, list(range(n))


def sparse_knapsack_milp_arrays(num_vars, num_cons, row_nonzeros, seed=0):
    """Sparse binary multi-knapsack: max c'x, W x <= cap, x in {0, 1}^n, every row with `row_nonzeros` integer
    weights in 5..30 on columns drawn without replacement, cap_i = floor(half the row's weight), c_j in 5..30; handed
    over as min -c'x, -W x >= -cap.  A family on which rounding is strong: lifted cover cuts (include/mipx_cover.h)
    close a large part of its root gap.  RNG: numpy Generator(PCG64(seed)), one row after the other, then c.

    Return (A, b, c, l, u, integer_indices) already in `min c'x, Ax >= b` form."""
    rng = np.random.Generator(np.random.PCG64(seed))
    n, m, k = int(num_vars), int(num_cons), int(row_nonzeros)
    W = np.zeros((m, n))
    for i in range(m):
        cols = rng.choice(n, size=k, replace=False)
        W[i, cols] = rng.integers(5, 31, k)
    cap = np.floor(0.5 * W.sum(1))
    c = rng.integers(5, 31, n).astype(np.float64)
    return -W, -cap, -c, np.zeros(n), np.ones(n), list(range(n))


def conflict_packing_milp_arrays(num_vars, num_edges, num_knapsacks, row_nonzeros, seed=0):
    """Binary packing with pairwise conflicts: max c'x over x in {0, 1}^n with `num_edges` rows x_i + x_j <= 1 and
    `num_knapsacks` rows W x <= cap of `row_nonzeros` integer weights in 5..30 on columns drawn without replacement,
    cap = floor(a quarter of the row's weight), c_j in 5..30; handed over as min -c'x, -W x >= -cap.  The LP relaxation
    of the pair rows sits at 0.5 and neither rounding a row nor covering it moves it: the family the clique cuts of
    include/mipx_clique.h are measured on.  RNG: numpy Generator(PCG64(seed)): the pairs (i, j), i < j, in
    lexicographic order, `num_edges` of them drawn without replacement and taken in ascending order; then one
    knapsack after the other (its columns, then its weights); then c.

    Return (A, b, c, l, u, integer_indices) already in `min c'x, Ax >= b` form."""
    rng = np.random.Generator(np.random.PCG64(seed))
    n, k = int(num_vars), int(row_nonzeros)
    pairs = [(i, j) for i in range(n) for j in range(i + 1, n)]
    pick = rng.choice(len(pairs), size=int(num_edges), replace=False)
    W = np.zeros((int(num_edges) + int(num_knapsacks), n))
    cap = np.ones(len(W))
    for r, q in enumerate(np.sort(pick)):
        W[r, list(pairs[q])] = 1.0
    for r in range(int(num_edges), len(W)):
        cols = rng.choice(n, size=k, replace=False)
        W[r, cols] = rng.integers(5, 31, k)
        cap[r] = np.floor(0.25 * W[r].sum())
    c = rng.integers(5, 31, n).astype(np.float64)
    return -W, -cap, -c, np.zeros(n), np.ones(n), list(range(n))
