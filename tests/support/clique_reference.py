"""NumPy restatement of include/mipx_clique.h: the conflict graph of the rows and the greedy clique separation of one
seed, from the header and not from the kernel.  The knapsack form is that of include/mipx_cover.h as
tests/support/cover_reference.py states it (the same expressions, its margin, the BLOCK SUM of
tests/support/mir_reference.py), nothing fused, so that the kernels can be compared with it: the graph, the statuses
and the sizes exactly, pi, pi0 and the efficacy bit for bit."""
import numpy as np

from tests.support.cover_reference import MARGIN, MIN_EFFICACY
from tests.support.mir_reference import block_sum

CUT, NO_CLIQUE, SHALLOW, SKIPPED = 0, 1, 2, 4
ROW_USED, ROW_SKIPPED = 0, 4


def words(n):
    return (2 * n + 31) // 32


def pack(B):
    """A boolean (2n, 2n) matrix as (2n, Wd) uint32 words: literal k is bit k mod 32 of word k div 32."""
    B = np.asarray(B, bool)
    k2 = B.shape[0]
    Wd = (k2 + 31) // 32
    pad = np.zeros((k2, 32 * Wd), np.uint64)
    pad[:, :k2] = B
    return (pad.reshape(k2, Wd, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)


def unpack(adj, n):
    """The (2n, Wd) words as a boolean (2n, 2n) matrix; the bits at 2n and above are dropped."""
    adj = np.asarray(adj, np.uint32)
    bits = (adj[:, :, None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)
    return bits.reshape(adj.shape[0], -1)[:, :2 * n].astype(bool)


def binary_columns(l, u, int_idx):
    """BINARY of mipx_cover.h, one flag per column."""
    l = np.asarray(l, np.float64); u = np.asarray(u, np.float64)
    isint = np.zeros(len(l), bool)
    isint[np.asarray(int_idx, dtype=np.int64)] = True
    with np.errstate(invalid='ignore'):
        return isint & (u < np.inf) & (np.floor(l) == l) & (np.floor(u) == u) & (u - l == 1.0)


def live_literals(l, u, int_idx):
    return np.repeat(binary_columns(l, u, int_idx), 2)


def knapsack_form(a_row, b_i, l, u, binary):
    """KNAPSACK FORM of one row a_row . x >= b_i: None when the row is skipped, else (literals, w, W, tau) of its
    items in column order."""
    a_row = np.asarray(a_row, np.float64)
    g = 0.0 - a_row
    part = g != 0.0
    item = part & binary
    with np.errstate(invalid='ignore'):
        bnd = np.where(g > 0.0, l, u)
        skip = part & ~item & ~(bnd < np.inf)
        K = block_sum(np.where(part & ~skip, g * np.where(skip, 0.0, bnd), 0.0))
    W = (0.0 - float(b_i)) - K
    if bool(np.any(skip)) or not W >= 0.0:
        return None
    cols = np.flatnonzero(item)
    return 2 * cols + (g[cols] < 0.0), np.abs(g[cols]), W, MARGIN * max(1.0, abs(W))


def graph(A, b, l, u, int_idx):
    """GRAPH: returns (adjacency as a boolean (2n, 2n) matrix, row status (m,))."""
    A = np.asarray(A, np.float64); b = np.asarray(b, np.float64)
    l = np.asarray(l, np.float64); u = np.asarray(u, np.float64)
    m, n = A.shape
    binary = binary_columns(l, u, int_idx)
    adj = np.zeros((2 * n, 2 * n), bool)
    status = np.zeros(m, np.int32)
    for i in range(m):
        form = knapsack_form(A[i], b[i], l, u, binary)
        if form is None:
            status[i] = ROW_SKIPPED
            continue
        lit, w, W, tau = form
        conflict = (w[:, None] + w[None, :]) - W > tau
        np.fill_diagonal(conflict, False)   # (two different items)
        e, f = np.nonzero(conflict)
        adj[lit[e], lit[f]] = True
    return adj, status


def literal_values(x, l, u, binary):
    """y* of the 2n literals at x: clipped to [0, 1], 0 for a literal that is not live."""
    x = np.asarray(x, np.float64)
    y = np.zeros(2 * len(x))
    with np.errstate(invalid='ignore'):
        y[0::2] = np.where(binary, np.clip(x - l, 0.0, 1.0), 0.0)
        y[1::2] = np.where(binary, np.clip(np.where(binary, u, 0.0) - x, 0.0, 1.0), 0.0)
    return y


def separate_seed(x, l, u, int_idx, adj, seed, min_efficacy=MIN_EFFICACY):
    """SEPARATION of one seed; adj a boolean (2n, 2n) matrix.  Returns dict(pi, pi0, efficacy, size, status, clique):
    clique the literals of Q in the order they were taken (None without a cut)."""
    x = np.asarray(x, np.float64); l = np.asarray(l, np.float64); u = np.asarray(u, np.float64)
    n = len(x)
    binary = binary_columns(l, u, int_idx)
    live = np.repeat(binary, 2)
    zero = dict(pi=np.zeros(n), pi0=0.0, efficacy=0.0, size=0, clique=None)
    seed = int(seed)
    if not live[seed]:
        return dict(zero, status=SKIPPED)
    y = literal_values(x, l, u, binary)
    if not y[seed] > 0.0:
        return dict(zero, status=NO_CLIQUE)
    Q = [seed]
    C = adj[seed] & live
    C[seed] = False
    while C.any():
        cand = np.flatnonzero(C)
        t = int(cand[np.argmax(y[cand])])   # (the first of the largest: the smallest literal number)
        Q.append(t)
        C = C & adj[t]
        C[t] = False
    if len(Q) < 2:
        return dict(zero, status=NO_CLIQUE)
    pi = np.zeros(n)
    for k in Q:
        pi[k >> 1] = 1.0 if k & 1 else 0.0 - 1.0
    with np.errstate(invalid='ignore'):
        T = block_sum(np.where(pi > 0.0, pi * np.where(pi > 0.0, u, 0.0), np.where(pi < 0.0, pi * l, 0.0)))
    pi0 = T - 1.0
    V, Qn = block_sum(pi * x), block_sum(pi * pi)
    eff = float((pi0 - V) / np.sqrt(Qn))
    return dict(pi=pi, pi0=float(pi0), efficacy=eff, size=len(Q), status=CUT if eff > min_efficacy else SHALLOW,
                clique=Q)


def separate(X, l, u, int_idx, adj, seeds=None, min_efficacy=MIN_EFFICACY):
    """The batch entry: X (batch, n), one box, adj boolean or packed; seeds None (the 2n literals) or R literals.
    Returns the kernel's outputs as arrays, (batch, R) each and (batch, R, n) for pi."""
    l = np.asarray(l, np.float64)
    n = len(l)
    X = np.asarray(X, np.float64).reshape(-1, n)
    adj = np.asarray(adj)
    if adj.dtype != bool:
        adj = unpack(adj, n)
    seeds = list(range(2 * n)) if seeds is None else [int(s) for s in seeds]
    B, R = X.shape[0], len(seeds)
    out = dict(pi=np.zeros((B, R, n)), pi0=np.zeros((B, R)), efficacy=np.zeros((B, R)),
               size=np.zeros((B, R), np.int32), status=np.zeros((B, R), np.int32))
    for p in range(B):
        for k, s in enumerate(seeds):
            res = separate_seed(X[p], l, u, int_idx, adj, s, min_efficacy)
            for name in out:
                out[name][p, k] = res[name]
    return out


def distinct_cuts(out, p=0):
    """The status-0 seeds of point p reduced to the distinct (pi, pi0), the first seed's kept: their places."""
    seen, places = set(), []
    for k in np.flatnonzero(out['status'][p] == CUT):
        key = (out['pi'][p, k].tobytes(), float(out['pi0'][p, k]))
        if key not in seen:
            seen.add(key)
            places.append(int(k))
    return places
