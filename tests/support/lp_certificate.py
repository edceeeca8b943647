"""Independent certificates for node-LP verdicts -- TEST INFRASTRUCTURE.

Imports no product code and no oracle code: a verdict (status, obj, x, y, vstat) of

    min c.x,  A x >= b,  l <= x <= u,      slack s = A x - b >= 0,
    vstat: 1 basic / 2 at upper / 3 at lower over the n structurals, then the m slacks

is checked against (A, b, c, l, u) alone, with matrix-vector products in arithmetic whose own error is
negligible: numpy.longdouble where it has a 64-bit mantissa, fractions.Fraction otherwise (and always
for the Farkas certificate of status 1).

Tolerances are the contract a verdict is taken under (oracle/mipx_oracle.c, "Clp defaults"), not new
numbers: PTOL = DTOL = 1e-7.  Derived per instance:
    slack     = 4 (n + m) eps (|c|.|x| + |b|.|y|)      rounding of the reported f64 dot product
    gap_bound = DTOL * sum_j (u_j - l_j over finite boxes) + PTOL * sum_i y_i + slack
(c.x - D(y) = y.s + sum_j [max(d_j,0)(x_j - l_j) + min(d_j,0)(x_j - u_j)]: each term is bounded by one
of the two tolerances times the quantity it multiplies.)

Three readings the contract needs and the checker takes (counted or printed in the report):
  * weak duality bounds D(y) by c.x' of a FEASIBLE x'.  The reported x is feasible to its residuals only,
    and D(y) may exceed c.x by exactly what they weigh, infeas = y.max(-s, 0) + |d|.max(l - x, x - u, 0),
    computed here from the measured residuals (1e-13 where the contract would allow PTOL sum_i y_i ~ 1e-6):
    the lower half of the sandwich is D(y) - slack - infeas <= obj;
  * a fixed variable (l_j == u_j) has no sign condition on d_j: its term in D(y) is d_j l_j either way;
  * where a bound is infinite, a d_j on its wrong side by at most DTOL is dual feasible under the
    contract; D(y) takes it as 0 there (`clipped`), otherwise D(y) would be -inf for every such LP.
"""
from fractions import Fraction

import numpy as np

PTOL = 1e-7
DTOL = 1e-7
EPS = float(np.finfo(np.float64).eps)
LONGDOUBLE_OK = np.finfo(np.longdouble).nmant >= 63
BASIC, UPPER, LOWER = 1, 2, 3
MREPORT = 1e10   # |x_j| at or above this: a variable reported on an infinite bound (status 2 / 3 only)


def _to_fraction(a):
    a = np.asarray(a, dtype=np.float64)
    out = np.empty(a.shape, dtype=object)
    flat = out.reshape(-1)
    for k, v in enumerate(a.reshape(-1)):
        flat[k] = Fraction(float(v))
    return out


def _to_longdouble(a):
    return np.asarray(a, dtype=np.float64).astype(np.longdouble)


def _f(a):
    """Values of the working arithmetic back as f64 (they are residuals and sums by then)."""
    return np.array([float(v) for v in np.asarray(a).reshape(-1)], dtype=np.float64).reshape(np.shape(a))


def measure(A, b, c, L, U, X, Y, V, exact=None):
    """Every quantity a certificate is judged by, for a batch of results of one (A, b, c): L, U, X
    (B, n), Y (B, m), V (B, n + m).  exact=True: Fraction; False: longdouble; None: longdouble where it
    has a 64-bit mantissa.  Returns a dict of f64 / int / bool arrays of length B."""
    if exact is None:
        exact = not LONGDOUBLE_OK
    conv = _to_fraction if exact else _to_longdouble
    A = np.asarray(A, np.float64); m, n = A.shape
    b = np.asarray(b, np.float64).reshape(m); c = np.asarray(c, np.float64).reshape(n)
    L = np.asarray(L, np.float64).reshape(-1, n); U = np.asarray(U, np.float64).reshape(-1, n)
    V = np.asarray(V).reshape(-1, n + m)
    B = len(V)
    X = np.asarray(X, np.float64).reshape(B, n); Y = np.asarray(Y, np.float64).reshape(B, m)
    vs, vr = V[:, :n], V[:, n:]
    finl, finu = np.isfinite(L), np.isfinite(U)
    A_, b_, c_, X_, Y_ = conv(A), conv(b), conv(c), conv(X), conv(Y)
    L_, U_ = conv(np.where(finl, L, 0.0)), conv(np.where(finu, U, 0.0))
    zero = conv(np.zeros(1))[0]

    S = X_ @ A_.T - b_                      # (B, m) slack of every row
    D = c_ - Y_ @ A_                        # (B, n) reduced costs
    Sf, Df = _f(S), _f(D)

    # primal side
    below = np.where(finl, _f(L_ - X_), -np.inf)
    above = np.where(finu, _f(X_ - U_), -np.inf)
    primal = np.maximum(0.0, np.max(np.concatenate([-Sf, below, above], axis=1), axis=1, initial=0.0))
    named = np.where(vs == UPPER, U, np.where(vs == LOWER, L, X))
    with np.errstate(invalid='ignore'):
        off = np.where(vs == BASIC, 0.0, np.abs(X - named))       # exact: both are f64 inputs
    off = np.where(np.isnan(off), np.inf, off)
    off_bound = np.max(off, axis=1, initial=0.0)
    slack_off = np.max(np.where(vr != BASIC, np.abs(Sf), 0.0), axis=1, initial=0.0)
    nbasic = np.sum(V == BASIC, axis=1)

    # dual side
    y_min = np.min(Y, axis=1, initial=0.0)
    y_basic = np.max(np.where(vr == BASIC, np.abs(Y), 0.0), axis=1, initial=0.0)
    fixed = finl & finu & (L == U)
    viol = np.where(vs == LOWER, -Df, np.where(vs == UPPER, Df, np.abs(Df)))
    viol = np.where(fixed, 0.0, viol)
    viol = np.maximum(viol, np.where(~finu & ~fixed, -Df, 0.0))   # u = inf: d_j >= -tol whatever vstat says
    viol = np.maximum(viol, np.where(~finl & ~fixed, Df, 0.0))
    dual = np.maximum(0.0, np.max(viol, axis=1, initial=0.0))

    # D(y) = b.y + sum_j (max(d_j, 0) l_j + min(d_j, 0) u_j)
    pos = Df > 0
    neg = Df < 0
    term = np.where(pos, D * L_, zero) + np.where(neg, D * U_, zero)
    hole = (pos & ~finl) | (neg & ~finu)                          # d_j on the side of an infinite bound
    clip = hole & (np.abs(Df) <= DTOL)
    term = np.where(hole, zero, term)
    Dy = Y_ @ b_ + (term.sum(axis=1) if n else zero)
    Dy = np.where(np.any(hole & ~clip, axis=1), -np.inf, _f(Dy))
    cx_ = X_ @ c_
    cx = _f(cx_)
    with np.errstate(invalid='ignore'):
        gap = np.where(np.isfinite(Dy), _f(cx_ - (Y_ @ b_ + (term.sum(axis=1) if n else zero))), np.inf)

    # weak duality holds for feasible points; the reported x misses feasibility by its residuals, and
    # D(y) may exceed c.x by exactly what they weigh: y.max(-s, 0) + |d|.max(l - x, x - u, 0)
    out_x = np.maximum(np.maximum(np.where(finl, _f(L_ - X_), 0.0), np.where(finu, _f(X_ - U_), 0.0)), 0.0)
    infeas = (np.maximum(Y, 0.0) * np.maximum(-Sf, 0.0)).sum(axis=1) + (np.abs(Df) * out_x).sum(axis=1)
    slack = 4.0 * (n + m) * EPS * (np.abs(X) @ np.abs(c) + np.abs(Y) @ np.abs(b))
    box = np.where(finl & finu, U - L, 0.0).sum(axis=1)
    gap_bound = DTOL * box + PTOL * np.maximum(Y, 0.0).sum(axis=1) + slack
    return dict(primal=primal, off_bound=off_bound, slack_off=slack_off, nbasic=nbasic, y_min=y_min,
                y_basic=y_basic, dual=dual, D=Dy, cx=cx, gap=gap, slack=slack, infeas=infeas, gap_bound=gap_bound,
                clipped=clip.sum(axis=1), on_inf=np.any(np.abs(X) >= MREPORT, axis=1), m=m, n=n, B=B)


class Report:
    """Worst figures and counts of one family of results; str() is the line a test prints."""

    KEYS = ('primal', 'dual', 'slack_off', 'rel_gap', 'obj_err', 'infeas')

    def __init__(self, family):
        self.family = family
        self.worst = {k: 0.0 for k in self.KEYS}
        self.count = {0: 0, 1: 0, 2: 0, 3: 0}
        self.farkas_verified = 0
        self.farkas_skipped = 0
        self.farkas_min_margin = np.inf
        self.status3_vacuous = 0
        self.clipped = 0

    def see(self, key, value):
        if np.size(value):
            self.worst[key] = max(self.worst[key], float(np.max(value)))

    def __str__(self):
        w = ' '.join(f'{k}={v:.3g}' for k, v in self.worst.items())
        return (f'[certificates] {self.family}: status 0/1/2/3 = {self.count[0]}/{self.count[1]}/{self.count[2]}/'
                f'{self.count[3]}; worst {w}; farkas verified {self.farkas_verified} skipped {self.farkas_skipped} '
                f'min margin {self.farkas_min_margin:.3g}; status-3 on an infinite bound {self.status3_vacuous}; '
                f'clipped d_j {self.clipped}')


def _fail(what, k, name, value, bound):
    raise AssertionError(f'{what} LP {k}: {name} = {value!r} violates {bound!r}')


def check_dual_half(M, k, what, status):
    """y >= 0, y_i == 0 on basic slacks, reduced costs signed as the basis says, exactly m basic."""
    if M['nbasic'][k] != M['m']:
        _fail(what, k, 'number of basic variables', int(M['nbasic'][k]), M['m'])
    if not M['y_min'][k] >= 0.0:
        _fail(what, k, 'min y', M['y_min'][k], '>= 0')
    if M['y_basic'][k] != 0.0:
        _fail(what, k, 'max |y_i| on a basic slack', M['y_basic'][k], '== 0')
    if not M['dual'][k] <= DTOL:
        _fail(what, k, f'reduced-cost sign violation (status {status})', M['dual'][k], f'<= {DTOL}')


def check_optimal(M, k, obj, what=''):
    """The optimality certificate of result k of a measured batch (status 0)."""
    if not M['primal'][k] <= PTOL:
        _fail(what, k, 'primal residual', M['primal'][k], f'<= {PTOL}')
    if M['off_bound'][k] != 0.0:
        _fail(what, k, 'distance of a nonbasic x_j from the bound vstat names', M['off_bound'][k], '== 0')
    if not M['slack_off'][k] <= PTOL:
        _fail(what, k, '|A x - b| on a nonbasic slack', M['slack_off'][k], f'<= {PTOL}')
    check_dual_half(M, k, what, 0)
    D, cx, slack = M['D'][k], M['cx'][k], M['slack'][k]
    if not np.isfinite(D):
        _fail(what, k, 'D(y)', D, 'finite')
    if not D - slack - M['infeas'][k] <= obj:
        _fail(what, k, 'obj - D(y)', obj - D, f'>= -({slack} + {M["infeas"][k]})')
    if not obj <= cx + slack:
        _fail(what, k, 'obj - c.x', obj - cx, f'<= {slack}')
    if not M['gap'][k] <= M['gap_bound'][k]:
        _fail(what, k, 'c.x - D(y)', M['gap'][k], f'<= {M["gap_bound"][k]}')


def check_truncated(M, k, obj, what='', optimum=None):
    """Status 3: the dual half only -- dual-feasible y, obj <= D(y) + slack, and D(y) <= the optimum of
    the same LP where the caller knows it (+inf: the LP is infeasible).  Returns False where a variable
    sits on an infinite bound (the basis is not dual feasible there, D(y) = -inf, nothing to certify)."""
    if M['on_inf'][k]:
        return False
    check_dual_half(M, k, what, 3)
    D, slack = M['D'][k], M['slack'][k]
    if not obj <= D + slack:
        _fail(what, k, 'obj - D(y) (status 3)', obj - D, f'<= {slack}')
    if optimum is not None and not D <= optimum + slack:
        _fail(what, k, 'D(y) - optimum (status 3)', D - optimum, f'<= {slack}')
    return True


def certify_batch(A, b, c, L, U, res, report, what='', exact=None, optimum=None, rows=None):
    """Certify every status-0 and status-3 row of `res` (dict of batch arrays; y may be missing: see
    duals_from_basis).  optimum: per-row optimum of the same LP for the status-3 rows, or None.
    Status 1 and 2 are counted only (certify_infeasible / the caller's HiGHS check).  Returns M."""
    status = np.asarray(res['status'])
    rows = np.arange(len(status)) if rows is None else np.asarray(rows)
    sel = rows[(status[rows] == 0) | (status[rows] == 3)]
    for s in (0, 1, 2, 3):
        report.count[s] += int(np.sum(status[rows] == s))
    if len(sel) == 0:
        return None
    L = np.asarray(L, np.float64).reshape(len(status), -1); U = np.asarray(U, np.float64).reshape(len(status), -1)
    M = measure(A, b, c, L[sel], U[sel], res['x'][sel], res['y'][sel], res['vstat'][sel], exact=exact)
    for k, r in enumerate(sel):
        tag = f'{what} row {r}'
        if status[r] == 0:
            check_optimal(M, k, res['obj'][r], tag)
            report.see('primal', M['primal'][k]); report.see('dual', M['dual'][k])
            report.see('slack_off', M['slack_off'][k])
            report.see('rel_gap', abs(M['gap'][k]) / max(1.0, abs(M['cx'][k])))
            report.see('obj_err', abs(res['obj'][r] - M['cx'][k])); report.see('infeas', M['infeas'][k])
            report.clipped += int(M['clipped'][k])
        else:
            ok = check_truncated(M, k, res['obj'][r], tag, None if optimum is None else optimum[r])
            if ok:
                report.see('dual', M['dual'][k])
                report.clipped += int(M['clipped'][k])
            else:
                report.status3_vacuous += 1
    return M


def duals_from_basis(A, c, vstat):
    """Row duals of the basis `vstat` in plain f64: B^T y = c_B over the columns of [A | -I] (a candidate,
    like the Farkas ray: the certificate then judges it).  y_i is set to exactly 0 where slack i is basic."""
    A = np.asarray(A, np.float64); m, n = A.shape
    vstat = np.asarray(vstat)
    basic = np.flatnonzero(vstat == BASIC)
    if len(basic) != m:
        raise AssertionError(f'{len(basic)} basic variables, {m} rows')
    Bm = np.hstack([A, -np.eye(m)])[:, basic]
    cB = np.where(basic < n, np.concatenate([np.asarray(c, np.float64), np.zeros(m)])[basic], 0.0)
    y = np.linalg.solve(Bm.T, cB)
    y[vstat[n:] == BASIC] = 0.0
    return y


def farkas_margin(A, b, l, u, rho):
    """Exact check of a Farkas candidate: every feasible point has rho.(A x - s) = rho.b, so the LP is
    infeasible if rho.b lies outside the exact range of rho.[A | -I] z over the box l <= x <= u, s >= 0.
    Returns the margin as a Fraction (> 0: proven infeasible), or None if the range is unbounded on
    both sides."""
    A = np.asarray(A, np.float64); m, n = A.shape
    rho_f = _to_fraction(rho)
    keep = np.flatnonzero(np.asarray(rho, np.float64) != 0.0)
    w = np.zeros(n, dtype=object) + Fraction(0)
    if len(keep):
        w = rho_f[keep] @ _to_fraction(A[keep])
    rb = sum((rho_f[i] * Fraction(float(b[i])) for i in keep), Fraction(0))
    lo = Fraction(0); hi = Fraction(0); lo_inf = hi_inf = False
    for j in range(n):
        if w[j] == 0:
            continue
        a, z = (l[j], u[j]) if w[j] > 0 else (u[j], l[j])     # a: where w_j z_j is smallest, z: largest
        if np.isfinite(a):
            lo += w[j] * Fraction(float(a))
        else:
            lo_inf = True
        if np.isfinite(z):
            hi += w[j] * Fraction(float(z))
        else:
            hi_inf = True
    for i in keep:                                            # slack column: -rho_i s_i, s_i in [0, inf)
        if rho_f[i] > 0:
            lo_inf = True
        else:
            hi_inf = True
    margins = []
    if not lo_inf:
        margins.append(lo - rb)
    if not hi_inf:
        margins.append(rb - hi)
    return max(margins) if margins else None


def certify_infeasible(A, b, l, u, vstat, tries=8):
    """Status 1.  The results carry no ray, so a candidate is derived from the reported basis in f64
    (B = [A | -I][:, basic], the basic values, the most violated rows r, rho = row r of B^-1) and then
    verified exactly.  Returns (margin as float, r) of the first verified candidate; raises with the
    best margin seen if none verifies; returns (None, None) if every candidate's range is unbounded."""
    A = np.asarray(A, np.float64); m, n = A.shape
    vstat = np.asarray(vstat)
    basic = np.flatnonzero(vstat == BASIC)
    if len(basic) != m:
        raise AssertionError(f'status 1 with {len(basic)} basic variables, {m} rows')
    full = np.hstack([A, -np.eye(m)])
    lo = np.concatenate([np.asarray(l, np.float64), np.zeros(m)])
    up = np.concatenate([np.asarray(u, np.float64), np.full(m, np.inf)])
    z = np.where(vstat == UPPER, up, lo)
    z = np.where(np.isfinite(z), z, np.where(np.isfinite(lo), lo, 0.0))
    z[basic] = 0.0
    Bm = full[:, basic]
    zB = np.linalg.solve(Bm, np.asarray(b, np.float64) - full @ z)
    viol = np.maximum(lo[basic] - zB, zB - up[basic])
    order = [r for r in np.argsort(-viol, kind='stable')[:tries] if viol[r] > 0]
    best = None
    for r in order:
        e = np.zeros(m); e[r] = 1.0
        rho = np.linalg.solve(Bm.T, e)
        for pos, v in enumerate(basic):          # row r of B^-1 is exactly 0 on every other basic slack's row
            if v >= n and pos != r:
                rho[v - n] = 0.0
        margin = farkas_margin(A, b, l, u, rho)
        if margin is not None and margin > 0:
            return float(margin), int(r)
        if margin is not None and (best is None or margin > best):
            best = margin
    if best is None and order:
        return None, None
    raise AssertionError(f'no Farkas certificate from the reported basis: best exact margin '
                         f'{None if best is None else float(best)!r} over {len(order)} violated rows '
                         f'(largest violation {float(np.max(viol, initial=0.0))!r})')


def certify_infeasible_rows(A, b, L, U, res, report, what='', boxed=True, highs_says_infeasible=None):
    """Every status-1 row of a batch.  boxed: every one must verify.  Otherwise a candidate whose range is
    unbounded may be skipped only if highs_says_infeasible(l, u) is True; the count is kept."""
    for r in np.flatnonzero(np.asarray(res['status']) == 1):
        margin, _ = certify_infeasible(A, b, L[r], U[r], res['vstat'][r])
        if margin is None:
            if boxed:
                raise AssertionError(f'{what} row {r}: unbounded Farkas range in a boxed family')
            if not highs_says_infeasible(L[r], U[r]):
                raise AssertionError(f'{what} row {r}: status 1, no certificate, and HiGHS does not say infeasible')
            report.farkas_skipped += 1
        else:
            report.farkas_verified += 1
            report.farkas_min_margin = min(report.farkas_min_margin, margin)
