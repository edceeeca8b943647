"""The reduced-cost bound tightening of include/mipx_rcfix.h restated in NumPy, one node at a time, in the order the
header states: products and subtractions rounded separately, yp . b summed rows ascending, the terms t_j through 256
partial sums and the fixed fold.  So l', u' and z are the kernel's bit for bit.  Also here: a brute-force validity
checker and the inputs the tests share (row duals by HiGHS, the cutoff of a shape).  Test infrastructure only."""
import itertools

import numpy as np
from scipy.optimize import linprog

UNCHANGED, TIGHTENED, CUT_OFF, NO_BOUND = 0, 1, 2, 3
TOL = 1e-6
DTOL = 1e-9
PARTIALS = 256


def bound_of(A, b, c, l, u, y):
    """(d, z) of steps 1 to 4."""
    m, n = A.shape
    yp = np.where(y > 0, y, 0.0)   # (a NaN compares false: +0)
    d = c.copy()
    for i in range(m):             # rows ascending; a row with yp_i = 0 changes nothing
        if yp[i] != 0.0:
            d = d - (A[i] * yp[i])
    with np.errstate(invalid='ignore'):   # (0 * inf in a branch that is not taken)
        t = np.where(d > 0, d * l, np.where(d < 0, d * u, 0.0))
    yb = 0.0
    for i in range(m):
        if yp[i] != 0.0:
            yb = yb + yp[i] * b[i]
    rows = -(-n // PARTIALS)
    pad = np.zeros(rows * PARTIALS)   # (the padding adds +0 to a partial that started from +0: the same bits)
    pad[:n] = t
    pad = pad.reshape(rows, PARTIALS)
    part = np.zeros(PARTIALS)
    with np.errstate(invalid='ignore'):
        for r in range(rows):         # partial k: its columns k, k + 256, ... ascending
            part = part + pad[r]
        s = PARTIALS // 2
        while s > 0:                  # the fold: p[k] += p[k + s] for k < s
            part[:s] = part[:s] + part[s:2 * s]
            s //= 2
        z = yb + part[0]
    return d, float(z)


def tighten_one(A, b, c, l, u, y, int_idx, cutoff, tol=TOL, dtol=DTOL):
    """(l', u', z, status, changed) of one box."""
    A = np.asarray(A, np.float64)
    b, c = np.asarray(b, np.float64), np.asarray(c, np.float64)
    l, u, y = np.array(l, dtype=np.float64), np.array(u, dtype=np.float64), np.asarray(y, np.float64)
    n = A.shape[1]
    d, z = bound_of(A, b, c, l, u, y)
    U = float(cutoff)
    if not np.isfinite(U) or np.isnan(z) or z == -np.inf:
        return l, u, z, NO_BOUND, 0
    g = U - z
    if g < -1e-6 * max(1.0, abs(U)):
        return l, u, z, CUT_OFF, 0
    if not g > 0.0:
        g = 0.0
    is_int = np.zeros(n, bool)
    is_int[np.asarray(int_idx, dtype=np.int64)] = True
    up_rule = is_int & (d > dtol)
    lo_rule = is_int & ~up_rule & (d < -dtol) & np.isfinite(u)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        vu = l + np.floor(g / d + tol)
        vl = u - np.floor(g / (-d) + tol)
        nu = np.where(up_rule & (vu < u), vu, u)
        nl = np.where(lo_rule & (vl > l), vl, l)
    changed = int(np.sum(nl != l) + np.sum(nu != u))
    return nl, nu, z, (TIGHTENED if changed > 0 else UNCHANGED), changed


def tighten(A, b, c, L, U, Y, int_idx, cutoff, tol=TOL, dtol=DTOL):
    """The batch: dict of l, u (B, n), z (B,), status, changed (B,) int32."""
    A = np.asarray(A, np.float64)
    m, n = A.shape
    L, U = np.asarray(L, np.float64).reshape(-1, n), np.asarray(U, np.float64).reshape(-1, n)
    B = L.shape[0]
    Y = np.asarray(Y, np.float64).reshape(B, m)
    out = dict(l=L.copy(), u=U.copy(), z=np.zeros(B), status=np.zeros(B, np.int32), changed=np.zeros(B, np.int32))
    for p in range(B):
        out['l'][p], out['u'][p], out['z'][p], out['status'][p], out['changed'][p] = \
            tighten_one(A, b, c, L[p], U[p], Y[p], int_idx, cutoff, tol, dtol)
    return out


def brute_force_check(A, b, c, l, u, cutoff, lo, up, status):
    """Over every integer point of the box l..u (small n, small bounds): the points with A x >= b and c . x <= cutoff
    all lie in lo..up, and status CUT_OFF is given only when there is none.  Returns the number of such points."""
    A, b, c = np.asarray(A, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64)
    P = np.array(list(itertools.product(*[range(int(lj), int(uj) + 1) for lj, uj in zip(l, u)])), dtype=np.float64)
    keep = np.all(P @ A.T >= b[None, :], axis=1) & (P @ c <= cutoff)
    if status == CUT_OFF:
        assert not keep.any(), 'cut off, but a point of the box satisfies the rows within the cutoff'
    if status in (CUT_OFF, NO_BOUND):
        assert np.array_equal(lo, l) and np.array_equal(up, u)
    assert np.all((P[keep] >= lo) & (P[keep] <= up)), 'a point within the cutoff was lost'
    assert np.all(lo >= l) and np.all(up <= u) and np.all(lo <= up)
    return int(keep.sum())


# ---- the inputs the tests share ------------------------------------------------------------------------------------
def highs_duals(A, b, c, L, U):
    """(Y, feasible): per box the duals of the rows A x >= b of min c . x over the box by HiGHS' dual simplex (zeros
    where the LP is infeasible), and which boxes were solved."""
    A = np.asarray(A, np.float64)
    m = A.shape[0]
    Y = np.zeros((len(L), m))
    feasible = np.zeros(len(L), bool)
    for p in range(len(L)):
        r = linprog(c, A_ub=-A, b_ub=-np.asarray(b), bounds=list(zip(L[p], U[p])), method='highs-ds')
        if r.status == 0:
            Y[p] = -r.ineqlin.marginals
            feasible[p] = True
    return Y, feasible


def cutoff_for(z, feasible):
    """The cutoff of a shape: the median of the bounds z of its LP-feasible boxes, rounded up."""
    return float(np.ceil(np.median(np.asarray(z)[np.asarray(feasible)])))


def boxes_of(n, m):
    """How many of propagation_reference.boxes() a shape takes (1000 x 700: the first 9)."""
    return 9 if n >= 1000 else 65


def dyadic_duals(m, count, seed=5):
    """Row duals in multiples of 1/8, about a third of them nonzero, some negative."""
    rng = np.random.default_rng(seed)
    return rng.integers(-8, 25, (count, m)) / 8.0 * (rng.random((count, m)) < 0.3)
