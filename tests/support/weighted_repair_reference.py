"""The weighted row repair of include/mipx_wrepair.h restated in NumPy, in the header's order of operations: every
sum is one add per term, rows ascending and columns ascending, products rounded on their own (np.add.accumulate adds
term after term along its axis, unlike np.sum, which adds in pairs).  Written from the header, not from the kernel.
Test infrastructure only."""
import numpy as np

FEASIBLE, CAPPED, SKIPPED = 0, 2, 3
MAX_STEPS = 256


def _weighted(s, w, tol):
    """Sum of w_i (-s_i) over s_i < -tol, rows ascending from +0; s is (m,) or (m, k) (one column per candidate)."""
    w = w if s.ndim == 1 else w[:, None]
    terms = np.where(s < -tol, w * (-s), 0.0)
    return np.add.accumulate(np.concatenate([np.zeros((1,) + s.shape[1:]), terms]), axis=0)[-1]


def weighted_repair_one(A, b, c, l, u, int_idx, x, tol=1e-9, max_steps=MAX_STEPS, trace=None):
    """(x~, obj, status, (moves, bumps)) of one point.  trace: a list that takes ('round', x~) once, then ('move', j, d)
    or ('bump',) per step."""
    A = np.asarray(A, np.float64)
    m, n = A.shape
    b, c, l, u = (np.asarray(v, np.float64) for v in (b, c, l, u))
    x = np.array(x, dtype=np.float64)
    J = np.asarray(int_idx, dtype=np.int64)
    xt = x.copy()
    lo, hi = np.ceil(l[J] - tol), np.floor(u[J] + tol)
    xt[J] = np.minimum(np.maximum(np.floor(xt[J] + 0.5), lo), hi) + 0.0   # ROUND (+ 0.0: a zero is +0)
    s = np.add.accumulate(np.hstack([np.zeros((m, 1)), A * xt[None, :]]), axis=1)[:, -1] - b
    w = np.ones(m)
    cJ, AJ = c[J], A[:, J]
    moves = bumps = 0
    if trace is not None:
        trace.append(('round', xt.copy()))
    while np.any(s < -tol):   # STEP
        if moves + bumps == max_steps:
            return x, 0.0, CAPPED, (moves, bumps)
        V = float(_weighted(s, w, tol))
        best = None
        for d in (1.0, -1.0):
            inside = (xt[J] + d >= lo) & (xt[J] + d <= hi)
            Vp = _weighted(s[:, None] + d * AJ, w, tol)
            for k in np.flatnonzero(inside):
                key = (float(Vp[k]), float(cJ[k] * d), int(J[k]), 0 if d > 0 else 1)
                if best is None or key < best:
                    best = key
        if best is not None and best[0] < V:
            j, d = best[2], (1.0 if best[3] == 0 else -1.0)
            xt[j] = xt[j] + d
            s = s + d * A[:, j]
            moves += 1
            if trace is not None:
                trace.append(('move', j, d))
        else:
            w = w + np.where(s < -tol, 1.0, 0.0)
            bumps += 1
            if trace is not None:
                trace.append(('bump',))
    obj = np.add.accumulate(np.concatenate([[0.0], c * xt]))[-1]
    return xt, float(obj), FEASIBLE, (moves, bumps)


def weighted_repair(A, b, c, l, u, int_idx, X, tol=1e-9, max_steps=MAX_STEPS, skip=None, gate=None):
    """The batch: dict of x (B, n), obj (B,), status (B,) int32 and counts (B, 2) int32 (moves, bumps); a skipped
    point (skip non-zero, or a gate entry that is not 1 or 2) comes back unchanged with obj 0, status 3 and no counts."""
    X = np.asarray(X, np.float64).reshape(-1, np.asarray(A).shape[1])
    B = X.shape[0]
    out = dict(x=X.copy(), obj=np.zeros(B), status=np.zeros(B, np.int32), counts=np.zeros((B, 2), np.int32))
    for p in range(B):
        if (skip is not None and skip[p]) or (gate is not None and gate[p] not in (1, 2)):
            out['status'][p] = SKIPPED
            continue
        out['x'][p], out['obj'][p], out['status'][p], out['counts'][p] = \
            weighted_repair_one(A, b, c, l, u, int_idx, X[p], tol, max_steps)
    return out


# ---- the instances, points and expected results the tests share ------------------------------------------------------
# (family, n, m, points, max_steps, tol, skip, gate, fixed): the smallest shapes at which the kernel takes another path
# (n below and not a multiple of a wave, m > n, more than one column per thread, the largest with a cap of 3); skip:
# every fifth point is skipped; gate: point p carries the status p % 4, so that 1 and 2 run and 0 and 3 do not; fixed:
# every seventh integer column has u = l (no candidate on it).  The guide points of a shape this large are not LP
# points and need no bump; the case named lp-points takes LP points there (fix_propagate_reference.lp_points), which do
CASES = {
    'generator-8x4': ('generator', 8, 4, 65, 256, 1e-9, False, False, False),
    'mixed-8x4-skip-gate': ('mixed', 8, 4, 65, 256, 1e-9, True, True, False),
    'generator-40x20-gate': ('generator', 40, 20, 65, 256, 1e-9, False, True, False),
    'mixed-40x20': ('mixed', 40, 20, 65, 256, 1e-9, False, False, False),
    'mixed-40x20-steps-4': ('mixed', 40, 20, 65, 4, 1e-9, False, False, False),
    'mixed-40x20-fixed-columns': ('mixed', 40, 20, 65, 64, 1e-6, False, False, True),
    'half-40x20-skip': ('half_continuous', 40, 20, 65, 256, 1e-9, True, False, False),
    'mixed-70x33': ('mixed', 70, 33, 65, 256, 1e-9, False, False, False),
    'half-70x33-gate': ('half_continuous', 70, 33, 3, 256, 1e-6, False, True, False),
    'generator-64x300': ('generator', 64, 300, 3, 256, 1e-9, False, False, False),
    'mixed-64x300-skip': ('mixed', 64, 300, 9, 256, 1e-9, True, False, False),
    'generator-300x150': ('generator', 300, 150, 3, 256, 1e-9, False, False, False),
    'mixed-300x150-skip-gate': ('mixed', 300, 150, 9, 256, 1e-9, True, True, False),
    'mixed-300x150-lp-points': ('mixed', 300, 150, 5, 256, 1e-9, False, False, False),
    'half-300x150': ('half_continuous', 300, 150, 3, 256, 1e-9, False, False, False),
    'generator-1000x700-steps-3': ('generator', 1000, 700, 3, 3, 1e-9, False, False, False),
}

_CACHE = {}


def case(name):
    """(A, b, c, l, u, ints, X, max_steps, tol, skip, gate, want) of a case, made once: want is weighted_repair's dict.
    The instances and guide points are those of the dive's tests (fix_propagate_reference.instance, .points)."""
    if name not in _CACHE:
        from tests.support import fix_propagate_reference as fp
        family, n, m, count, max_steps, tol, with_skip, with_gate, fixed = CASES[name]
        A, b, c, l, u, ints = fp.instance(family, n, m)
        ints = np.asarray(ints, dtype=np.int64)
        if fixed:
            u = np.array(u, dtype=np.float64)
            u[ints[::7]] = np.asarray(l)[ints[::7]]
        X = fp.lp_points(A, b, c, l, u, ints, count) if name.endswith('lp-points') else fp.points(A, b, c, l, u, ints, count)
        skip = (np.arange(count) % 5 == 4).astype(np.uint8) if with_skip else None
        gate = (np.arange(count) % 4).astype(np.int32) if with_gate else None
        want = weighted_repair(A, b, c, l, u, ints, X, tol=tol, max_steps=max_steps, skip=skip, gate=gate)
        _CACHE[name] = (A, b, c, l, u, ints, X, max_steps, tol, skip, gate, want)
    return _CACHE[name]
