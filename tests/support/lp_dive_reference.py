"""The LP dive of include/mipx_lpdive.h restated in NumPy: PREPARE, STEP and FINISH in the header's order, around an LP
solver passed in as a function.  Each round is ONE call of that function over all the points, as the kernel's round is
one launch.  With the oracle's lp_solve_batch as that function -- which the node-LP kernels match bit for bit -- the
kernels give the same bits: STEP compares and copies, and FINISH is the completion's (completion_reference.finish_one).
Test infrastructure only."""
import numpy as np

from tests.support import completion_reference as comp

FEASIBLE, INFEASIBLE, LIMIT, SKIPPED, REJECTED, CUTOFF = 0, 1, 2, 3, 4, 5
FRACTIONAL, COEFFICIENT = 0, 1
FTOL = CTOL = 1e-6
ACTIVE, FINAL, PENDING, ENDED = 0, 1, 2, 3
KEYS = ('x', 'obj', 'status', 'rounds', 'fixings', 'flips', 'pivots')


def locks(A, int_idx):
    """(down, up) by position in int_idx: the rows with a positive and with a negative coefficient."""
    A = np.asarray(A, np.float64)
    J = np.asarray(int_idx, dtype=np.int64)
    return (A[:, J] > 0).sum(axis=0), (A[:, J] < 0).sum(axis=0)


def dive(A, b, c, L0, U0, int_idx, X, lp_solve, vstat=None, skip=None, cutoff=np.inf, max_rounds=64, rule=FRACTIONAL):
    """The batch.  L0, U0: (batch, n) or (n,).  lp_solve(L, U, V) solves min c.x, A x >= b, L_k <= x <= U_k for every
    row k from the basis codes V[k] ((n + m) int8; all 0: no basis) and returns a dict with status (0 optimal,
    1 infeasible, anything else: limit or unbounded), obj, x, vstat and npivots.  Returns dict(x, obj, status, rounds,
    fixings, flips, pivots)."""
    A = np.asarray(A, np.float64)
    m, n = A.shape
    X = np.asarray(X, np.float64).reshape(-1, n)
    B = X.shape[0]
    L0 = np.array(np.broadcast_to(np.asarray(L0, np.float64), (B, n)))
    U0 = np.array(np.broadcast_to(np.asarray(U0, np.float64), (B, n)))
    J = np.asarray(int_idx, dtype=np.int64)
    down, up = locks(A, J)
    xo, obj = X.copy(), np.zeros(B)
    status = np.full(B, LIMIT, np.int32)
    rounds, fixings, flips, pivots = (np.zeros(B, np.int32) for _ in range(4))
    if B == 0:
        return dict(x=xo, obj=obj, status=status, rounds=rounds, fixings=fixings, flips=flips, pivots=pivots)
    # PREPARE
    L, U = L0.copy(), U0.copy()
    V = np.zeros((B, n + m), np.int8)
    phase = np.full(B, ACTIVE)
    rec = [None] * B
    xcur = X.copy()
    for p in range(B):
        lo, hi = L0[p, J], U0[p, J]
        bad = (skip is not None and bool(np.asarray(skip)[p])) or not np.all(np.isfinite(X[p])) or \
            not np.all(np.isfinite(lo)) or not np.all(np.isfinite(hi)) or \
            np.any(np.abs(lo - np.rint(lo)) > CTOL) or np.any(np.abs(hi - np.rint(hi)) > CTOL)
        if bad:
            U[p] = L0[p]
            phase[p] = ENDED
            status[p] = SKIPPED
            continue
        L[p, J] = np.rint(lo)
        U[p, J] = np.rint(hi)
        if vstat is not None:
            V[p] = np.asarray(vstat, np.int8).reshape(B, n + m)[p]

    def end(p, code):
        L[p] = L0[p]; U[p] = L0[p]; V[p] = 0
        if code is None:
            phase[p] = PENDING
        else:
            phase[p] = ENDED
            status[p] = code

    r = None
    for rnd in range(1, max_rounds + 2):
        last = rnd > max_rounds
        live = 0
        for p in range(B):
            if phase[p] >= PENDING:
                continue
            select = True
            if rnd > 1:
                lp = r['status'][p]
                pivots[p] += r['npivots'][p]
                if lp == 0:
                    V[p] = r['vstat'][p]
                    xcur[p] = r['x'][p]
                    if not (r['obj'][p] < cutoff):
                        end(p, CUTOFF)
                        continue
                    if phase[p] == FINAL:
                        cand = xcur[p].copy()
                        cand[J] = L[p, J]
                        xo[p] = cand
                        end(p, None)
                        continue
                elif lp != 1:
                    end(p, LIMIT)
                    continue
                elif rec[p] is None:
                    end(p, INFEASIBLE)
                    continue
                elif last:
                    end(p, LIMIT)
                    continue
                else:   # FLIP
                    j, oldL, oldU, v, xj = rec[p]
                    lo, hi = (v + 1.0, oldU) if v <= xj else (oldL, v - 1.0)
                    if lo > hi:
                        end(p, INFEASIBLE)
                        continue
                    L[p, j], U[p, j] = lo, hi
                    rec[p] = None
                    flips[p] += 1
                    select = False
            if select and last:
                end(p, LIMIT)
                continue
            if select:
                x = xcur[p]
                best = None   # (lock, frac, position)
                for k, j in enumerate(J):
                    if not (L[p, j] < U[p, j]):
                        continue
                    f = abs(x[j] - np.rint(x[j]))
                    if not (f > FTOL):
                        continue
                    key = (int(min(down[k], up[k])) if rule == COEFFICIENT else 0, f, k)
                    if best is None or key < best:
                        best = key
                if best is None:
                    for j in J:
                        if L[p, j] < U[p, j]:
                            v = min(max(np.floor(x[j] + 0.5), L[p, j]), U[p, j])
                            L[p, j] = U[p, j] = v
                    phase[p] = FINAL
                    rec[p] = None
                else:
                    k = best[2]
                    j = J[k]
                    v = np.floor(x[j] + 0.5)
                    if rule == COEFFICIENT:
                        if down[k] < up[k]:
                            v = np.floor(x[j])
                        elif up[k] < down[k]:
                            v = np.ceil(x[j])
                    v = min(max(v, L[p, j]), U[p, j])
                    rec[p] = (j, L[p, j], U[p, j], v, x[j])
                    L[p, j] = U[p, j] = v
                    fixings[p] += 1
            rounds[p] += 1
            live += 1
        if last or live == 0:
            break
        r = lp_solve(L.copy(), U.copy(), V.copy())
    # FINISH
    for p in range(B):
        if phase[p] != PENDING:
            continue
        xo[p], obj[p], st = comp.finish_one(A, b, c, L0[p], U0[p], J, xo[p], xo[p], CTOL)
        status[p] = FEASIBLE if st == comp.COMPLETED else REJECTED
        if st != comp.COMPLETED:
            xo[p] = X[p]
    return dict(x=xo, obj=obj, status=status, rounds=rounds, fixings=fixings, flips=flips, pivots=pivots)


def oracle_lp(A, b, c):
    """The oracle's node LP as the restatement's LP function."""
    from oracle import oracle as O
    return lambda L, U, V: O.lp_solve_batch(A, b, c, L, U, V)


_CACHE = {}


def profile_points(inst, seed, count=64, moved=4):
    """(X, V, L, U) by the recipe of lp_points in scripts/completion_profile.py, with the oracle's node LP: the root's LP
    point, then rounds of `count` LPs with `moved` random integer bounds each moved to the floor (as upper bound) or the
    ceil (as lower bound) of the root value, warm from the root's basis, of which the optimal ones are kept in order;
    with every point its final basis codes and its node's box.  Made once per instance."""
    key = (inst[0].tobytes(), inst[1].tobytes(), seed, count, moved)
    if key not in _CACHE:
        A, b, c, l, u, ints = inst
        lp = oracle_lp(A, b, c)
        n, m = len(c), len(b)
        root = lp(l[None], u[None], np.zeros((1, n + m), np.int8))
        assert root['status'][0] == 0
        rng = np.random.default_rng(seed)
        X, V, Ls, Us = [root['x'][0]], [root['vstat'][0]], [l.copy()], [u.copy()]
        for _ in range(50):
            L, U = np.tile(l, (count, 1)), np.tile(u, (count, 1))
            for k in range(count):
                for j in rng.choice(ints, size=moved, replace=False):
                    if rng.integers(0, 2):
                        U[k, j] = np.floor(root['x'][0, j])
                    else:
                        L[k, j] = np.ceil(root['x'][0, j])
            r = lp(L, U, np.repeat(root['vstat'], count, axis=0))
            for k in np.flatnonzero(r['status'] == 0):
                X.append(r['x'][k]); V.append(r['vstat'][k]); Ls.append(L[k]); Us.append(U[k])
            if len(X) >= count:
                break
        assert len(X) >= count, 'too few optimal LPs'
        _CACHE[key] = (np.array(X[:count]), np.array(V[:count], dtype=np.int8), np.array(Ls[:count]), np.array(Us[:count]))
    return _CACHE[key]
