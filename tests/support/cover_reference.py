"""NumPy restatement of include/mipx_cover.h: the lifted cover separation of one row, every sum in the header's order
(PREFIX SUM: 4 consecutive positions per thread, the scan inside each wave, then the waves in order; BLOCK SUM: that
of tests/support/mir_reference.py), nothing fused, so that the kernel can be compared with it bit for bit."""
import numpy as np

from tests.support.mir_reference import NT, WAVE, block_sum

CUT, NO_COVER, SHALLOW, SKIPPED = 0, 1, 2, 4
MARGIN = 1e-9
MIN_EFFICACY = 1e-6
PER = 4   # positions per thread
_LANES = np.arange(WAVE)


def prefix_sum(terms):
    """The PREFIX SUM of the header over len(terms) <= 1024 positions: the value behind every position."""
    k = len(terms)
    pad = np.zeros(NT * PER)
    pad[:k] = terms
    s = np.zeros((NT, PER))
    t = np.zeros(NT)
    for c in range(PER):
        t = t + pad.reshape(NT, PER)[:, c]   # (a position past the end adds +0: the same bits as not adding)
        s[:, c] = t
    inc = t.reshape(NT // WAVE, WAVE).copy()
    for off in (1, 2, 4, 8, 16, 32):
        below = np.zeros_like(inc)
        below[:, off:] = inc[:, :-off]
        inc = np.where(_LANES >= off, inc + below, inc)
    exc = np.zeros_like(inc)
    exc[:, 1:] = inc[:, :-1]
    T = inc[:, WAVE - 1]
    base = np.array([0.0, T[0], T[0] + T[1], (T[0] + T[1]) + T[2]])
    start = (base[:, None] + exc).reshape(NT)
    return (start[:, None] + s).reshape(-1)[:k]


def separate_row(a_row, b_i, x, l, u, int_idx, min_efficacy=MIN_EFFICACY):
    """One row a_row . x >= b_i at the point x in the box l, u.  Returns dict(pi, pi0, efficacy, cover_size, status,
    cover, alpha): cover the columns of C, alpha the coefficients of the items by column (both None without a cut)."""
    a_row = np.asarray(a_row, np.float64); x = np.asarray(x, np.float64)
    l = np.asarray(l, np.float64); u = np.asarray(u, np.float64)
    n = len(a_row)
    isint = np.zeros(n, bool)
    isint[np.asarray(int_idx, dtype=np.int64)] = True
    zero = dict(pi=np.zeros(n), pi0=0.0, efficacy=0.0, cover_size=0, cover=None, alpha=None)
    g = 0.0 - a_row
    part = g != 0.0
    with np.errstate(invalid='ignore'):
        binary = part & isint & (u < np.inf) & (np.floor(l) == l) & (np.floor(u) == u) & (u - l == 1.0)
        bnd = np.where(g > 0.0, l, u)
        skip = part & ~binary & ~(bnd < np.inf)
        K = block_sum(np.where(part & ~skip, g * np.where(skip, 0.0, bnd), 0.0))
    W = (0.0 - float(b_i)) - K
    if bool(np.any(skip)) or not W >= 0.0:
        return dict(zero, status=SKIPPED)
    tau = MARGIN * max(1.0, abs(W))
    cols = np.flatnonzero(binary)   # item e is column cols[e]
    nb = len(cols)
    if nb < 2:
        return dict(zero, status=NO_COVER)
    comp = g[cols] < 0.0
    w = np.abs(g[cols])
    y = np.where(comp, u[cols] - x[cols], x[cols] - l[cols])
    y = np.where(y < 0.0, 0.0, np.where(y > 1.0, 1.0, y))
    key = (1.0 - y) / w
    # GREEDY COVER
    order = np.lexsort((np.arange(nb), key))   # (key, e) ascending
    P = prefix_sum(w[order])
    hit = np.flatnonzero(P - W > tau)
    if len(hit) == 0:
        return dict(zero, status=NO_COVER)
    c0 = order[:hit[0] + 1]
    # MINIMAL COVER: (w descending, e descending)
    c0 = c0[np.lexsort((-c0, -w[c0]))]
    mu = prefix_sum(w[c0])
    hit = np.flatnonzero(mu - W > tau)
    if len(hit) == 0:
        return dict(zero, status=NO_COVER)
    r = int(hit[0]) + 1
    C = c0[:r]
    # LIFTING
    thr = mu[:r] + MARGIN * np.maximum(1.0, mu[:r])
    alpha = (w[:, None] >= thr[None, :]).sum(axis=1).astype(np.float64)
    alpha[C] = 1.0
    # OUTPUT
    pi = np.zeros(n)
    pi[cols] = np.where(comp, alpha, 0.0 - alpha)
    with np.errstate(invalid='ignore'):
        T = block_sum(np.where(pi > 0.0, pi * np.where(pi > 0.0, u, 0.0), np.where(pi < 0.0, pi * l, 0.0)))
    pi0 = T - float(r - 1)
    V, Q = block_sum(pi * x), block_sum(pi * pi)
    eff = float((pi0 - V) / np.sqrt(Q))
    by_col = np.zeros(n)
    by_col[cols] = alpha
    return dict(pi=pi, pi0=float(pi0), efficacy=eff, cover_size=r, status=CUT if eff > min_efficacy else SHALLOW,
                cover=np.sort(cols[C]), alpha=by_col)


def separate(A, b, X, L, U, int_idx, rows=None, min_efficacy=MIN_EFFICACY):
    """The batch entry: X, L, U (batch, n); rows None (the m rows) or R row indices.  Returns the kernel's outputs as
    arrays, (batch, R) each and (batch, R, n) for pi."""
    A = np.asarray(A, np.float64); b = np.asarray(b, np.float64)
    m, n = A.shape
    X = np.asarray(X, np.float64).reshape(-1, n); L = np.asarray(L, np.float64).reshape(-1, n)
    U = np.asarray(U, np.float64).reshape(-1, n)
    rows = list(range(m)) if rows is None else [int(i) for i in rows]
    B, R = X.shape[0], len(rows)
    out = dict(pi=np.zeros((B, R, n)), pi0=np.zeros((B, R)), efficacy=np.zeros((B, R)),
               cover_size=np.zeros((B, R), np.int32), status=np.zeros((B, R), np.int32))
    for p in range(B):
        for k, i in enumerate(rows):
            res = separate_row(A[i], b[i], X[p], L[p], U[p], int_idx, min_efficacy)
            for name in out:
                out[name][p, k] = res[name]
    return out
