"""NumPy restatement of include/mipx_mir.h: the MIR separation of one base row, every sum in the header's order (WAVE
SUM: lanes stride the columns, then the butterfly; BLOCK SUM: threads stride the columns, the butterfly inside each
wave, then the waves in order), nothing fused, so that the kernel can be compared with it bit for bit."""
import numpy as np

CUT, NO_TRIAL, SHALLOW, DYNAMISM, SKIPPED = 0, 1, 2, 3, 4
NT, WAVE = 256, 64
INSIDE = 1e-6
TINY = 1e-9
MAX_DIVISORS, F0_MIN, MIN_EFFICACY, MAX_DYNAMISM = 16, 0.05, 1e-8, 1e6
_LANES = np.arange(WAVE)


def _butterfly(v):
    """v: (..., 64) lane values; v += shfl_xor(v, off) for off = 32 .. 1."""
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[..., _LANES ^ off]
    return v


def _strided(terms, width):
    """Thread q adds terms q, q + width, ... in that order to +0: (width,) partial sums."""
    k = len(terms)
    pad = np.zeros(-(-max(k, 1) // width) * width)
    pad[:k] = terms
    part = np.zeros(width)
    for chunk in pad.reshape(-1, width):
        part = part + chunk
    return part


def wave_sum(terms):
    return float(_butterfly(_strided(terms, WAVE))[0])


def block_sum(terms):
    w = _butterfly(_strided(terms, NT).reshape(NT // WAVE, WAVE))[:, 0]
    return float(((w[0] + w[1]) + w[2]) + w[3])


def _row_sum(start, weights, M):
    """One thread per column: start + sum_i w_i M[i], rows in row order, rows with w_i = 0 left out."""
    acc = np.array(start, dtype=np.float64, copy=True)
    for i in np.flatnonzero(weights != 0.0):
        acc = acc + weights[i] * M[i]
    return acc


def _coef(part, isint, gs, delta, f0, omf):
    with np.errstate(all='ignore'):
        a = gs / delta
        fa = np.floor(a)
        r = (a - fa) - f0
        ki = fa + np.where(r > 0.0, r, 0.0) / omf
        kc = np.where(gs < 0.0, gs / (delta * omf), 0.0)
    return np.where(part, np.where(isint, ki, kc), 0.0)


def separate_row(A, b, x, l, u, int_idx, row_integral, lam, max_divisors=MAX_DIVISORS, f0_min=F0_MIN,
                 min_efficacy=MIN_EFFICACY, max_dynamism=MAX_DYNAMISM):
    """One base row lam (m multipliers) at the point x in the box l, u.  Returns dict(pi, pi0, efficacy, delta, sign,
    status, candidates, index): candidates the divisor list, index (k, h) with delta = candidates[k] / 2**h."""
    A = np.asarray(A, np.float64); b = np.asarray(b, np.float64)
    x = np.asarray(x, np.float64); l = np.asarray(l, np.float64); u = np.asarray(u, np.float64)
    lam = np.asarray(lam, np.float64)
    m, n = A.shape
    N = n + m
    rint = np.zeros(m, bool) if row_integral is None else np.asarray(row_integral).astype(bool)
    isint = np.zeros(N, bool)
    isint[np.asarray(int_idx, dtype=np.int64)] = True
    g0 = np.zeros(N); ts = np.zeros(N); part = np.zeros(N, bool); elig = np.zeros(N, bool); comp = np.zeros(N, bool)
    # slack columns of the rows with a multiplier
    for i in np.flatnonzero(lam != 0.0):
        sv = wave_sum(A[i] * x) - b[i]
        st = sv if sv > 0.0 else 0.0
        g0[n + i] = 0.0 - lam[i]
        ts[n + i] = st
        part[n + i] = True
        isint[n + i] = rint[i]
        elig[n + i] = rint[i] and st > INSIDE
    d0 = float(_row_sum(0.0, lam, b))
    # structural columns
    g = _row_sum(np.zeros(n), lam, A)
    fin = u < np.inf
    with np.errstate(invalid='ignore'):
        cx = fin & (u - x < x - l)
        tx = np.where(cx, u - x, x - l)
        bnd = np.where(cx, u, l)
        px = g != 0.0
        ex = px & isint[:n] & (tx > INSIDE) & (~fin | ((u - l) - tx > INSIDE))
    skipped = bool(np.any(px & isint[:n] & (np.floor(bnd) != bnd)))
    g0[:n] = g; ts[:n] = tx; part[:n] = px; elig[:n] = ex; comp[:n] = cx
    gp = np.where(comp, 0.0 - g0, g0)
    bound = np.concatenate([bnd, np.zeros(m)])
    dp = d0 - block_sum(g0 * bound)
    G = float(np.abs(gp).max())
    noise = isint & (np.abs(gp) <= TINY * G)
    isint = isint & ~noise
    elig = elig & ~noise
    # the divisor list
    cands = []
    for j in np.flatnonzero(elig):
        if len(cands) >= max_divisors:
            break
        v = abs(gp[j])
        if v not in cands:
            cands.append(v)
    if 1.0 not in cands:
        cands.append(1.0)
    zero = dict(pi=np.zeros(n), pi0=0.0, efficacy=0.0, delta=0.0, sign=0, candidates=cands, index=None)
    if skipped:
        return dict(zero, status=SKIPPED)

    def trial(sg, delta):
        beta = (sg * dp) / delta
        flb = np.floor(beta)
        f0 = beta - flb
        if not (G / delta <= max_dynamism and abs(beta) <= max_dynamism):
            return None
        if not (f0 >= f0_min and f0 <= 1.0 - f0_min):
            return None
        k = _coef(part, isint, sg * gp, delta, f0, 1.0 - f0)
        P, Q = block_sum(k * ts), block_sum(k * k)
        if not Q > 0.0:
            return None
        with np.errstate(all='ignore'):
            eff = (P - flb) / np.sqrt(Q)
        return float(eff) if np.isfinite(eff) else None

    low = np.concatenate([l, np.zeros(m)])
    upp = np.concatenate([u, np.full(m, np.inf)])

    def cut_of(sg, delta):
        beta = (sg * dp) / delta
        flb = np.floor(beta)
        f0 = beta - flb
        k = _coef(part, isint, sg * gp, delta, f0, 1.0 - f0)
        with np.errstate(invalid='ignore'):
            cterm = np.where(comp, 0.0 - k * np.where(comp, upp, 0.0), k * low)
        nu = flb + block_sum(cterm)
        mu = np.where(comp, 0.0 - k, k)
        pi0 = 0.0 - float(_row_sum(nu, mu[n:], b))
        pi = 0.0 - _row_sum(mu[:n], mu[n:], A)
        V, W = block_sum(pi * x), block_sum(pi * pi)
        effx = float((pi0 - V) / np.sqrt(W)) if W > 0.0 else 0.0
        return pi, pi0, effx

    best = None   # (x-space efficacy, pi, pi0, delta, sign, index)
    for sg in (1.0, -1.0):
        sbest = None   # (efficacy of the trial, delta, index)
        for k, delta in enumerate(cands):
            eff = trial(sg, delta)
            if eff is not None and (sbest is None or eff > sbest[0]):
                sbest = (eff, delta, (k, 0))
        if sbest is None:
            continue
        star, kstar = sbest[1], sbest[2][0]
        for h in (1, 2, 3):
            delta = star / float(2 << (h - 1))
            eff = trial(sg, delta)
            if eff is not None and eff > sbest[0]:
                sbest = (eff, delta, (kstar, h))
        pi, pi0, effx = cut_of(sg, sbest[1])
        if best is None or effx > best[0]:
            best = (effx, pi, pi0, sbest[1], 1 if sg > 0 else -1, sbest[2])
    if best is None:
        return dict(zero, status=NO_TRIAL)
    effx, pi, pi0, delta, sign, index = best
    ap = np.abs(pi)
    mx = float(ap.max()) if n else 0.0
    mn = float(ap[ap != 0.0].min()) if np.any(ap != 0.0) else np.inf
    status = CUT
    if not effx > min_efficacy:
        status = SHALLOW
    elif mx / mn > max_dynamism:
        status = DYNAMISM
    return dict(pi=pi, pi0=pi0, efficacy=effx, delta=delta, sign=sign, status=status, candidates=cands, index=index)


def separate(A, b, X, L, U, int_idx, row_integral=None, multipliers=None, rows=None, **params):
    """The batch entry: X, L, U (batch, n); multipliers None (the m unit rows) or (R, m).  rows: only these base rows
    (the others' outputs stay 0 with status -1).  Returns the kernel's outputs as arrays."""
    A = np.asarray(A, np.float64)
    m, n = A.shape
    X = np.asarray(X, np.float64).reshape(-1, n); L = np.asarray(L, np.float64).reshape(-1, n)
    U = np.asarray(U, np.float64).reshape(-1, n)
    M = np.eye(m) if multipliers is None else np.asarray(multipliers, np.float64).reshape(-1, m)
    B, R = X.shape[0], M.shape[0]
    out = dict(pi=np.zeros((B, R, n)), pi0=np.zeros((B, R)), efficacy=np.zeros((B, R)), delta=np.zeros((B, R)),
               sign=np.zeros((B, R), np.int32), status=np.full((B, R), -1, np.int32), index={})
    for p in range(B):
        for r in (range(R) if rows is None else rows):
            res = separate_row(A, b, X[p], L[p], U[p], int_idx, row_integral, M[r], **params)
            for key in ('pi', 'pi0', 'efficacy', 'delta', 'sign', 'status'):
                out[key][p, r] = res[key]
            out['index'][p, r] = res['index']
    return out
