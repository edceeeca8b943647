"""The primal heuristic of include/mipx_heur.h restated in NumPy, in the header's order of operations: every sum
is one add per term, rows ascending and columns ascending, products rounded on their own (np.add.accumulate adds
term after term along its axis, unlike np.sum, which adds in pairs).  On integer data all of it is exact; elsewhere
the kernel, which takes the same order without fused multiply-adds, gives the same bits.  Test infrastructure only."""
import numpy as np

FEASIBLE, STUCK, CAPPED, SKIPPED = 0, 1, 2, 3


def _violation(s, tol):
    """Sum of -s_i over s_i < -tol, rows ascending; s is (m,) or (m, k) (one column per candidate)."""
    return np.add.accumulate(np.where(s < -tol, -s, 0.0), axis=0)[-1]


def round_repair_lift_one(A, b, c, l, u, int_idx, x, tol=1e-9, max_moves=None):
    """(x~, obj, status, (repair moves, lift moves)) of one point."""
    A = np.asarray(A, np.float64)
    m, n = A.shape
    b, c, l, u = (np.asarray(v, np.float64) for v in (b, c, l, u))
    J = np.asarray(int_idx, dtype=np.int64)
    max_moves = m + n if max_moves is None else int(max_moves)
    xt = np.array(x, dtype=np.float64)
    lo, hi = np.ceil(l[J] - tol), np.floor(u[J] + tol)
    xt[J] = np.minimum(np.maximum(np.floor(xt[J] + 0.5), lo), hi) + 0.0   # (+ 0.0: a zero is +0, as the header says)
    s = np.add.accumulate(np.hstack([np.zeros((m, 1)), A * xt[None, :]]), axis=1)[:, -1] - b   # (sums start at +0)
    cJ, AJ = c[J], A[:, J]
    repair = lift = 0
    status = FEASIBLE
    while np.any(s < -tol) and repair < max_moves:
        V = float(_violation(s, tol))
        best = None
        for d in (1.0, -1.0):
            inside = (xt[J] + d >= lo) & (xt[J] + d <= hi)
            Vp = _violation(s[:, None] + d * AJ, tol)
            for k in np.flatnonzero(inside & (Vp < V)):
                key = (float(Vp[k]), float(cJ[k] * d), int(J[k]), 0 if d > 0 else 1)
                if best is None or key < best:
                    best = key
        if best is None:
            status = STUCK
            break
        j, d = best[2], (1.0 if best[3] == 0 else -1.0)
        xt[j] = xt[j] + d
        s = s + d * A[:, j]
        repair += 1
    if status == FEASIBLE and np.any(s < -tol):
        status = CAPPED
    while status == FEASIBLE and repair + lift < max_moves:
        best = None
        for d in (1.0, -1.0):
            inside = (xt[J] + d >= lo) & (xt[J] + d <= hi)
            keeps = np.all(s[:, None] + d * AJ >= -tol, axis=0)
            for k in np.flatnonzero(inside & keeps & (cJ * d < 0)):
                key = (float(cJ[k] * d), int(J[k]), 0 if d > 0 else 1)
                if best is None or key < best:
                    best = key
        if best is None:
            break
        j, d = best[1], (1.0 if best[2] == 0 else -1.0)
        xt[j] = xt[j] + d
        s = s + d * A[:, j]
        lift += 1
    obj = np.add.accumulate(np.concatenate([[0.0], c * xt]))[-1]
    return xt, float(obj), status, (repair, lift)


def round_repair_lift(A, b, c, l, u, int_idx, X, tol=1e-9, max_moves=None, skip=None):
    """The batch: (X~ (B, n), obj (B,), status (B,) int32, moves (B, 2) int32); a skipped point comes back
    unchanged with obj 0, status 3 and no moves."""
    X = np.asarray(X, np.float64).reshape(-1, np.asarray(A).shape[1])
    B = X.shape[0]
    Xt, obj = X.copy(), np.zeros(B)
    status, moves = np.zeros(B, np.int32), np.zeros((B, 2), np.int32)
    for p in range(B):
        if skip is not None and skip[p]:
            status[p] = SKIPPED
            continue
        Xt[p], obj[p], status[p], moves[p] = round_repair_lift_one(A, b, c, l, u, int_idx, X[p], tol, max_moves)
    return Xt, obj, status, moves


def certify(A, b, c, l, u, int_idx, xt, obj, tol=1e-9, int_tol=0.0, obj_tol=1e-9):
    """Independent check of a point the heuristic calls feasible: rows, bounds, integrality, obj = c . x~ (with
    NumPy's own dot products, not the restatement's sums).  The defaults are the heuristic's own: its points are
    integral exactly; the solution of a search may come from a node LP and is checked with that suite's figures."""
    A, xt = np.asarray(A, np.float64), np.asarray(xt, np.float64)
    J = np.asarray(int_idx, dtype=np.int64)
    scale = max(1.0, float(np.max(np.abs(A) @ np.abs(xt))) if A.size else 1.0)
    assert np.all(A @ xt - np.asarray(b) >= -tol - 1e-12 * scale), 'a row is violated'
    assert np.all(xt >= np.asarray(l) - tol) and np.all(xt <= np.asarray(u) + tol), 'a bound is violated'
    assert np.all(np.abs(xt[J] - np.round(xt[J])) <= int_tol), 'an integer column is fractional'
    assert abs(float(np.asarray(c) @ xt) - obj) <= obj_tol * max(1.0, abs(obj)), 'obj is not c . x'
