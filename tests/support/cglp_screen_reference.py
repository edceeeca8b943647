"""The dual screen of a support evaluation, restated in NumPy (test infrastructure only): the weak-duality bound
L_t(pi; y+) in the arithmetic include/mipx_cglp_screen.h fixes, the screened rule and the packed order -- what
mipx_support_screen_batch must give bit for bit -- and a session without a GPU whose leaf LPs are HiGHS, for the
in-out logic of DisjunctiveSeparator.  Nothing here uses the engine.

NumPy has no fused multiply-add, so fma() builds one from error-free transformations (Boldo and Melquiond, Emulation
of a FMA and correctly rounded sums: proved algorithms using rounding to odd, IEEE TC 57(4), 2008): the product as an
exact pair, two exact sums, the two small parts added with rounding to odd, one last rounding.  Exact where nothing
overflows or falls below the normal range; tests/test_cglp_screen_abi.py checks it against rational arithmetic."""
import numpy as np
from scipy.optimize import linprog

LANES = 64


def _split(a):
    c = 134217729.0 * a            # 2^27 + 1 (Veltkamp)
    hi = c - (c - a)
    return hi, a - hi


def _two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _odd_sum(a, b):
    """a + b rounded to odd: the exact sum if it is a double, else the neighbour whose last bit is 1."""
    s, e = _two_sum(a, b)
    even = (np.ascontiguousarray(s).view(np.int64) & 1) == 0
    return np.where((e != 0) & even, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)


def fma(a, b, c):
    """a * b + c with one rounding, elementwise (an infinite or NaN operand: what a * b + c gives, as a fused one does)."""
    a, b, c = np.broadcast_arrays(*(np.asarray(v, np.float64) for v in (a, b, c)))
    with np.errstate(all='ignore'):
        plain = a * b + c
        uh, ul = _two_prod(a, b)
        th, tl = _two_sum(c, ul)
        vh, vl = _two_sum(uh, th)
        return np.where(np.isfinite(plain), vh + _odd_sum(tl, vl), plain)


def _butterfly(v):
    """v: (T, 64) partial sums -> (T,) their sum in the order of six rounds of xor-shuffles, offsets 32 .. 1."""
    idx = np.arange(LANES)
    off = LANES // 2
    while off:
        v = v + v[:, idx ^ off]
        off //= 2
    return v[:, 0]


def _lane_sums(terms):
    """terms: (T, k) -> (T, 64): lane q adds, from 0, entries q, q + 64, ... in ascending order."""
    T, k = terms.shape
    acc = np.zeros((T, LANES))
    for start in range(0, k, LANES):
        part = terms[:, start:start + LANES]
        acc[:, :part.shape[1]] = acc[:, :part.shape[1]] + part
    return acc


def bound(A, b, pi, l, u, y, has_y=None):
    """L_t(pi; y+) of every leaf: l, u (T, n), y (T, m); -inf where has_y is 0."""
    A, b, pi = (np.asarray(v, np.float64) for v in (A, b, pi))
    l, u, y = (np.atleast_2d(np.asarray(v, np.float64)) for v in (l, u, y))
    T, n = l.shape
    m = len(b)
    with np.errstate(all='ignore'):
        yp = np.where(y > 0.0, y, 0.0)
        s = np.zeros((T, n))
        for i in range(m):
            rows = np.flatnonzero(yp[:, i] > 0.0)
            if len(rows):
                s[rows] = fma(A[i][None, :], yp[rows, i][:, None], s[rows])
        r = pi[None, :] - s
        p1, p2 = r * l, r * u
        cols = _butterfly(_lane_sums(np.where(p2 < p1, p2, p1)))
        rows_sum = _butterfly(_lane_sums(yp * b[None, :])) if m else np.zeros(T)
        L = cols + rows_sum
    if has_y is not None:
        L = np.where(np.asarray(has_y) != 0, L, -np.inf)
    return L


def screen(A, b, pi, pi0, screen_tol, l, u, y, has_y):
    """dict(bound, screened, packed, count) as mipx_support_screen_batch gives them."""
    L = bound(A, b, pi, l, u, y, has_y)
    with np.errstate(all='ignore'):
        scr = (np.asarray(has_y) != 0) & np.isfinite(L) & (L - pi0 >= -screen_tol)
    keep = np.flatnonzero(~scr).astype(np.int32)
    packed = np.full(len(L), -1, np.int32)
    packed[:len(keep)] = keep
    return dict(bound=L, screened=scr.astype(np.uint8), packed=packed, count=len(keep))


def support_with_duals(pi, A, b, lo, up):
    """(status, h_t(pi), a minimiser, the row duals y >= 0 of A x >= b) by HiGHS."""
    res = linprog(pi, A_ub=-A, b_ub=-b, bounds=list(zip(lo, up)), method='highs')
    if res.status != 0:
        return res.status, None, None, None
    return 0, float(res.fun), np.asarray(res.x, np.float64), -np.asarray(res.ineqlin.marginals, np.float64)


def highs_tree(A, b, c, l, u, ints, leaves):
    """A best-first branch and bound on the most fractional column by HiGHS, stopped at `leaves` open nodes: the root's
    LP solution and the boxes (L, U) of the open nodes, which are all LP-feasible and cover the root's integer points."""
    def lp(lo, up):
        res = linprog(c, A_ub=-A, b_ub=-b, bounds=list(zip(lo, up)), method='highs')
        return (float(res.fun), np.asarray(res.x)) if res.status == 0 else None

    root = lp(l, u)
    x_root = root[1]
    open_nodes = [(root[0], root[1], np.array(l, np.float64), np.array(u, np.float64))]
    closed = []   # (integral leaves stay terms of the disjunction)
    while open_nodes and len(open_nodes) + len(closed) < leaves:
        open_nodes.sort(key=lambda nd: nd[0])
        obj, x, lo, up = open_nodes.pop(0)
        frac = np.abs(x[ints] - np.round(x[ints]))
        if frac.max() < 1e-6:
            closed.append((obj, x, lo, up))
            continue
        j = ints[int(np.argmax(frac))]
        for side in (0, 1):
            lo2, up2 = lo.copy(), up.copy()
            if side == 0:
                up2[j] = np.floor(x[j])
            else:
                lo2[j] = np.ceil(x[j])
            child = lp(lo2, up2)
            if child is not None:
                open_nodes.append((child[0], child[1], lo2, up2))
    nodes = open_nodes + closed
    return x_root, np.array([nd[2] for nd in nodes]), np.array([nd[3] for nd in nodes])


class HighsSession:
    """What DisjunctiveSeparator.on_session takes for an _ffi.Support session, with HiGHS for the leaf LPs and the
    restated screen: eval, stats, leaves.  Every leaf must be feasible."""

    def __init__(self, A, b, L, U, ids=None):
        self.A, self.b, self.L, self.U = (np.asarray(v, np.float64) for v in (A, b, L, U))
        self.ids = np.arange(len(self.L), dtype=np.int64) if ids is None else np.asarray(ids, np.int64)
        T, n = self.L.shape
        self.y = np.zeros((T, len(self.b)))
        self.has_y = np.zeros(T, np.uint8)
        self.x = np.zeros((T, n))
        self.lps = self.evals = self.screened = 0

    def eval(self, pi, pi0, tol=0.0, max_points=1, want_margins=False, screen_tol=None, retry_cold=False):
        T = len(self.ids)
        pi = np.asarray(pi, np.float64)
        h = np.zeros(T)
        scr = np.zeros(T, bool)
        if screen_tol is not None and self.evals:
            out = screen(self.A, self.b, pi, pi0, screen_tol, self.L, self.U, self.y, self.has_y)
            scr, h = out['screened'] != 0, out['bound'].copy()
        for t in np.flatnonzero(~scr):
            status, h[t], self.x[t], y = support_with_duals(pi, self.A, self.b, self.L[t], self.U[t])
            assert status == 0, (t, status)
            if screen_tol is not None:
                self.y[t], self.has_y[t] = y, 1
        solved = int((~scr).sum())
        self.lps += solved
        self.screened += T - solved
        self.evals += 1
        margins = h - pi0
        order = np.lexsort((self.ids, margins))[:max_points]
        res = dict(min_margin=float(margins.min()), min_id=int(self.ids[order[0]]), below=int((margins < -tol).sum()),
                   not_optimal=0, iterations=0, pivots=0, leaves=T, ids=self.ids[order], h=h[order], x=self.x[order].copy())
        if want_margins:
            res['margins'] = margins
        if screen_tol is not None or retry_cold:
            res.update(screened=T - solved, lp_solved=solved, retried=0, retried_optimal=0, screen_us=0.0,
                       min_screened_margin=float(margins[scr].min()) if scr.any() else float('inf'))
        return res

    def stats(self):
        return dict(leaves=len(self.ids), dropped=0, evaluations=self.evals, leaf_lps=self.lps, iterations=0, pivots=0,
                    device_bytes=0, kernel_ms=0.0, select_ms=0.0)

    def leaves(self, dropped=False):
        return np.zeros(0, np.int64) if dropped else self.ids.copy()

    def close(self):
        pass


def highs_master(self, X, x_star, basis):
    """DisjunctiveSeparator._solve_master by HiGHS (the engine's needs a GPU): min x*.pi - pi0 over X pi - pi0 >= 0,
    -1 <= pi <= 1, -R <= pi0 <= R.  Returns what the method returns; the basis is the mask of slack rows."""
    n, R = self.n, self.R
    cost = np.concatenate([x_star, [-1.0]])
    A_ub = -np.hstack([X, -np.ones((len(X), 1))])
    res = linprog(cost, A_ub=A_ub, b_ub=np.zeros(len(X)), bounds=[(-1.0, 1.0)] * n + [(-R, R)], method='highs')
    if res.status != 0:
        return None
    pi, pi0 = np.clip(res.x[:n], -1.0, 1.0), float(res.x[n])
    slack = (np.asarray(res.ineqlin.residual) > 1e-9).astype(np.int8)
    return pi, pi0, float(x_star @ pi - pi0), slack == 1, (np.zeros(n + 1, np.int8), slack)
