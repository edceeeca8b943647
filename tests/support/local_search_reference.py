"""The pair-move local search of include/mipx_lsearch.h restated in NumPy, in the header's order of operations:
s_i = a_i . x - b_i one add per term with the columns ascending from +0 (np.add.accumulate adds term after term along
its axis, unlike np.sum, which adds in pairs), a pair's row test as (s_i + dj a_ij) + dk a_ik, nothing fused.  The
kernel takes the same order, so the two agree bit for bit on any data.  The candidates of a move are filtered row by
row, the way the kernel's live flags die, the tightest rows first, and what survives those in the order of the keys:
which candidates survive every row does not depend on the order the rows are taken in.
Test infrastructure only."""
import numpy as np

LOCAL_OPT, CAPPED, NOT_FEASIBLE, SKIPPED = 0, 1, 2, 3
DIRS = ((0, 1.0), (1, -1.0))   # (+1 sorts before -1)
FIRST_ROWS, CHUNK = 16, 1024     # (how the candidates of a move are sifted: it changes the work, not the result)


def rounded_bounds(l, u, int_idx, tol):
    J = np.asarray(int_idx, dtype=np.int64)
    return np.ceil(np.asarray(l, np.float64)[J] - tol), np.floor(np.asarray(u, np.float64)[J] + tol)


def slacks(A, b, x):
    m = A.shape[0]
    return np.add.accumulate(np.hstack([np.zeros((m, 1)), A * x[None, :]]), axis=1)[:, -1] - b   # (sums start at +0)


def best_move(A, c, s, x, lo, hi, tol):
    """The smallest key (g, j, k, dj bit, dk bit) over the candidates at x, or None.  lo, hi: n each, with the empty
    range [1, 0] on the columns that are not integer."""
    m, n = A.shape
    room = {0: np.flatnonzero((x + 1.0 >= lo) & (x + 1.0 <= hi)), 1: np.flatnonzero((x - 1.0 >= lo) & (x - 1.0 <= hi))}
    order = np.argsort(s, kind='stable')   # (the survivors of all rows do not depend on the order the rows are taken in)
    best = None
    for djb, dj in DIRS:
        g = c * dj
        idx = room[djb][g[room[djb]] < 0]
        if idx.size:
            ok = np.all(s[:, None] + dj * A[:, idx] >= -tol, axis=0)
            for j in idx[ok]:
                key = (float(g[j]), int(j), -1, djb, 0)
                if best is None or key < best:
                    best = key
        for dkb, dk in DIRS:
            rj, rk = room[djb], room[dkb]
            if rj.size == 0 or rk.size == 0:
                continue
            gj, gk = c[rj] * dj, c[rk] * dk
            alive = (rj[:, None] < rk[None, :]) & (gj[:, None] + gk[None, :] < 0)
            a, e = np.nonzero(alive)
            jj, kk = rj[a], rk[e]
            for i in order[:FIRST_ROWS]:
                if jj.size == 0:
                    break
                keep = (s[i] + dj * A[i, jj]) + dk * A[i, kk] >= -tol
                jj, kk = jj[keep], kk[keep]
            if jj.size == 0:
                continue
            # ... then the rest in the order of their keys, a chunk at a time through the remaining rows: the first
            # survivor is the smallest key of this (dj, dk)
            gg = c[jj] * dj + c[kk] * dk
            by_key = np.lexsort((kk, jj, gg))
            jj, kk, gg, rest = jj[by_key], kk[by_key], gg[by_key], order[FIRST_ROWS:]
            for at in range(0, jj.size, CHUNK):
                cj, ck = jj[at:at + CHUNK], kk[at:at + CHUNK]
                ok = np.all((s[rest, None] + dj * A[np.ix_(rest, cj)]) + dk * A[np.ix_(rest, ck)] >= -tol, axis=0)
                if ok.any():
                    q = at + int(np.argmax(ok))
                    key = (float(gg[q]), int(jj[q]), int(kk[q]), djb, dkb)
                    if best is None or key < best:
                        best = key
                    break
    return best


def pair_search_one(A, b, c, l, u, int_idx, x, tol=1e-9, max_moves=64):
    """(x', obj, status, (single moves, pair moves)) of one point."""
    A = np.asarray(A, np.float64)
    m, n = A.shape
    b, c = np.asarray(b, np.float64), np.asarray(c, np.float64)
    J = np.asarray(int_idx, dtype=np.int64)
    x = np.array(x, dtype=np.float64)
    lo, hi = np.ones(n), np.zeros(n)
    lo[J], hi[J] = rounded_bounds(l, u, J, tol)
    s = slacks(A, b, x)
    objective = lambda v: float(np.add.accumulate(np.concatenate([[0.0], c * v]))[-1])   # noqa: E731
    if np.any(s < -tol) or np.any(x[J] != np.floor(x[J])) or not np.all((x[J] >= lo[J]) & (x[J] <= hi[J])):
        return x, objective(x), NOT_FEASIBLE, (0, 0)
    singles = pairs = 0
    while True:
        key = best_move(A, c, s, x, lo, hi, tol)
        if key is None:
            status = LOCAL_OPT
            break
        if singles + pairs >= max_moves:
            status = CAPPED
            break
        _, j, k, djb, dkb = key
        dj, dk = DIRS[djb][1], DIRS[dkb][1]
        x[j] = x[j] + dj
        s = s + dj * A[:, j]
        if k >= 0:
            x[k] = x[k] + dk
            s = s + dk * A[:, k]
            pairs += 1
        else:
            singles += 1
    return x, objective(x), status, (singles, pairs)


def pair_search(A, b, c, l, u, int_idx, X, tol=1e-9, max_moves=64, skip=None):
    """The batch: (X' (B, n), obj (B,), status (B,) int32, moves (B, 2) int32); a skipped point comes back unchanged
    with obj 0, status 3 and no moves."""
    X = np.asarray(X, np.float64).reshape(-1, np.asarray(A).shape[1])
    B = X.shape[0]
    Xo, obj = X.copy(), np.zeros(B)
    status, moves = np.zeros(B, np.int32), np.zeros((B, 2), np.int32)
    for p in range(B):
        if skip is not None and skip[p]:
            status[p] = SKIPPED
            continue
        Xo[p], obj[p], status[p], moves[p] = pair_search_one(A, b, c, l, u, int_idx, X[p], tol, max_moves)
    return Xo, obj, status, moves
