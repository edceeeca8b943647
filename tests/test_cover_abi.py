"""The lifted cover separation (include/mipx_cover.h), the parts that need no GPU: the header against the ctypes table
and the exported symbols, the NumPy restatement (tests/support/cover_reference.py) worked by hand, the minimality of
its covers, the validity of its cuts by exhaustion over every point of 3 000 knapsacks and by HiGHS on rows that mix
column kinds inside a node's box, the instance family, and the root cut loop with the cover option on the restatement
with HiGHS LPs."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest
from scipy.optimize import Bounds, LinearConstraint, linprog, milp

from simple_mip_solver_amd import _ffi
from simple_mip_solver_amd.generators import random_dense_milp_arrays, sparse_knapsack_milp_arrays
from simple_mip_solver_amd.utils import mir_cuts
from tests.support import cover_reference as ref
from tests.support import mir_reference
from tests.support.abi_check import agrees, prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float('inf')
NAME = 'mipx_cover_separate_batch'


def test_header_and_signature_table_agree():
    protos = prototypes('mipx_cover.h')
    assert sorted(protos) == sorted(_ffi.COVER_SYMBOLS) == [NAME]
    ret, params = protos[NAME]
    restype, argtypes = _ffi._COVER_SIGNATURES[NAME]
    assert agrees(ret, restype) and len(params) == len(argtypes) == 15
    for k, (decl, ctype) in enumerate(zip(params, argtypes)):
        assert agrees(decl, ctype), f'{NAME} parameter {k} is `{decl}`, the table says {ctype}'


def test_new_symbol_overlaps_no_existing_list():
    old = set()
    for attr in dir(_ffi):
        if attr.endswith('SYMBOLS') and attr != 'COVER_SYMBOLS':
            old |= set(getattr(_ffi, attr))
    assert old and not set(_ffi.COVER_SYMBOLS) & old


def test_mipx_h_includes_the_header_and_the_library_exports_its_entry():
    text = open(os.path.join(ROOT, 'include', 'mipx.h')).read()
    assert '#include "mipx_cover.h"' in text
    L = _ffi.lib()
    assert L.mipx_abi_version() == 1
    assert hasattr(L, NAME) and getattr(L, NAME).restype is C.c_int
    assert L.mipx_cover_separate_batch(None, 1, *([None] * 4), 0, None, 0, 1e-6, *([None] * 5)) == -1   # MIPX_EINVAL


def test_status_codes_cover_the_header():
    text = open(os.path.join(ROOT, 'include', 'mipx_cover.h')).read()
    codes = {name: int(v) for name, v in re.findall(r'#define MIPX_COVER_(\w+) (\d+)', text)}
    assert sorted(codes.values()) == sorted(_ffi.COVER_STATUS) == [0, 1, 2, 4]
    assert (codes['CUT'], codes['NO_COVER'], codes['SHALLOW'], codes['SKIPPED']) == \
        (ref.CUT, ref.NO_COVER, ref.SHALLOW, ref.SKIPPED)


def test_the_prefix_sum_follows_the_stated_order():
    """Numbers whose sums depend on the order: inside a thread, across the lanes of a wave, across the waves."""
    t = np.zeros(1024)
    t[0], t[1], t[2] = 1e16, 1.0, 1.0          # thread 0: (1e16 + 1) + 1 = 1e16 (each 1 is lost)
    t[4], t[5] = 1.0, 1.0                      # thread 1: 2, scanned onto thread 0's 1e16: 1e16 + 2
    t[256], t[257] = 3.0, 1.0                  # wave 1, thread 64: 3, then 4
    P = ref.prefix_sum(t)
    assert P[2] == 1e16 and P[3] == 1e16
    assert P[4] == 1e16 + 1.0 == 1e16 and P[5] == 1e16 + 2.0
    T0 = 1e16 + 2.0
    assert P[255] == T0 and P[256] == T0 + 3.0 and P[257] == T0 + 4.0 and P[1023] == T0 + 4.0
    w = np.arange(1.0, 301.0)
    assert np.array_equal(ref.prefix_sum(w), np.cumsum(w))   # (small integers: every order gives the same)
    assert len(ref.prefix_sum(np.ones(1))) == 1


def test_the_restatement_worked_by_hand():
    """3 xa + 3 xb + 3 xc - 7 xd <= 1 on binaries: xd is complemented (yd = 1 - xd, weight 7) and the capacity is
    W = 1 + 7 = 8.  At x* = (1, 1, 0.9, 0.95) the keys are (0, 0, 0.1/3, 0.95/7), the greedy prefix sums 3, 6, 9 > 8:
    C0 = {a, b, c}; mu = (3, 6, 9), so r = 3 and C = C0.  yd weighs 7 >= mu_1, mu_2 and < mu_3: alpha_d = 2.  The cut
    ya + yb + yc + 2 yd <= 2 is -xa - xb - xc + 2 xd >= -2 + 2 = 0."""
    a, b = [-3.0, -3.0, -3.0, 7.0], -1.0
    x, l, u = [1.0, 1.0, 0.9, 0.95], [0.0] * 4, [1.0] * 4
    r = ref.separate_row(a, b, x, l, u, [0, 1, 2, 3])
    assert r['status'] == ref.CUT and r['cover_size'] == 3 and r['cover'].tolist() == [0, 1, 2]
    assert np.array_equal(r['pi'], [-1.0, -1.0, -1.0, 2.0]) and r['pi0'] == 0.0 and r['alpha'].tolist() == [1, 1, 1, 2]
    assert abs(r['efficacy'] - 1.0 / np.sqrt(7.0)) < 1e-15
    # a general integer with g > 0 is relaxed out at l = 0, a continuous column with g = -1 at u = 2 (W gains 2, the
    # right-hand side takes it back): the same knapsack and the same cut, 0 on the two columns
    r2 = ref.separate_row(a + [-2.0, 1.0], 1.0, x + [3.0, 0.5], l + [0.0, 0.0], u + [5.0, 2.0], [0, 1, 2, 3, 4])
    assert r2['status'] == ref.CUT and np.array_equal(r2['pi'], [-1.0, -1.0, -1.0, 2.0, 0.0, 0.0]) and r2['pi0'] == 0.0
    # shifted boxes: binaries on {2, 3}: pi0 = -(r - 1) - sum alpha l + sum alpha u = -2 - 6 + 6
    r3 = ref.separate_row(a, b - 3.0 * 2 * 3 + 7.0 * 2, np.array(x) + 2.0, [2.0] * 4, [3.0] * 4, [0, 1, 2, 3])
    assert r3['status'] == ref.CUT and np.array_equal(r3['pi'], r['pi']) and r3['pi0'] == -2.0 - 6.0 + 6.0
    # the statuses: no cover (the whole row fits), fewer than two binaries, a shallow cut, an infinite bound, W < 0
    assert ref.separate_row(a, -10.0, x, l, u, [0, 1, 2, 3])['status'] == ref.NO_COVER
    assert ref.separate_row(a, b, x, l, u, [3])['status'] == ref.NO_COVER
    assert ref.separate_row([-3.0, -3.0], 1.0, [0.0, 0.0], [0.0, 0.0], [1.0, 1.0], [0, 1])['status'] == ref.SKIPPED
    sh = ref.separate_row(a, b, [0.5, 0.5, 0.5, 0.5], l, u, [0, 1, 2, 3])
    assert sh['status'] == ref.SHALLOW and sh['pi'].any() and sh['efficacy'] <= 1e-6 and sh['cover_size'] >= 1
    sk = ref.separate_row(a + [1.0], b, x + [0.0], l + [0.0], u + [INF], [0, 1, 2, 3])
    assert sk['status'] == ref.SKIPPED and not sk['pi'].any() and sk['cover_size'] == 0
    assert ref.separate_row(a + [-1.0], b, x + [0.0], l + [0.0], u + [INF], [0, 1, 2, 3])['status'] == ref.CUT
    # exact ties in key and weight end at the item number: every y* = 1, weights 2: C0 is the first three items; an
    # item outside that weighs exactly mu_1 stays at 0 (the margin of the comparison)
    tie = ref.separate_row([-2.0] * 5, -5.0, [1.0] * 5, [0.0] * 5, [1.0] * 5, range(5))
    assert tie['status'] == ref.CUT and tie['cover'].tolist() == [0, 1, 2] and tie['alpha'].tolist() == [1, 1, 1, 0, 0]
    # ... and of the three equal weights of C0 = {0, 1, 2, 3} the removal keeps the highest number
    tie = ref.separate_row([-1.0, -1.0, -1.0, -4.0], -4.5, [1.0] * 4, [0.0] * 4, [1.0] * 4, range(4))
    assert tie['cover'].tolist() == [2, 3] and tie['cover_size'] == 2 and tie['alpha'].tolist() == [0, 0, 1, 1]


# ---- minimality and validity by exhaustion -------------------------------------------------------------------------

WEIGHTS = np.array([1.0, 2.0, 3.0, 5.0, 8.0, 13.0, 40.0, 90.0])
NB = 12
POINTS = np.array(list(itertools.product((0.0, 1.0), repeat=NB)))


def single_row(rng):
    """One knapsack over 12 binaries as a row a . x >= b, and a point with exact 0s and 1s mixed in: weights from
    WEIGHTS, negative with probability 1/4, the capacity at 20 to 80 % of the range g . x can reach."""
    g = rng.choice(WEIGHTS, NB) * np.where(rng.random(NB) < 0.25, -1.0, 1.0)
    lo, hi = g[g < 0].sum(), g[g > 0].sum()
    d = np.floor(lo + rng.uniform(0.2, 0.8) * (hi - lo))
    y = rng.random(NB)
    kind = rng.random(NB)
    y = np.where(kind < 0.45, 1.0, np.where(kind < 0.6, 0.0, y))   # (in item space: most items of a root LP sit at 1)
    x = np.where(g < 0, 1.0 - y, y)
    return 0.0 - g, 0.0 - d, x


def test_minimality_removing_any_item_leaves_no_cover():
    rng = np.random.default_rng(5)
    seen = 0
    for _ in range(300):
        a, b, x = single_row(rng)
        r = ref.separate_row(a, b, x, np.zeros(NB), np.ones(NB), range(NB))
        if r['cover'] is None:
            continue
        g = 0.0 - a
        W = (0.0 - b) - g[g < 0].sum()
        w = np.abs(g)[r['cover']]
        assert len(w) == r['cover_size'] and w.sum() > W            # (integers: exact)
        assert np.all(w.sum() - w <= W), (w, W)
        assert np.all(r['alpha'][r['cover']] == 1.0)
        seen += 1
    assert seen >= 150, seen


def test_exhaustive_validity_of_3000_single_rows():
    """No cut is violated at any of the 2^12 points of its knapsack (integer data: the check is exact), and the sample
    is not a tame one: lifted coefficients of 2 and more and complemented columns occur often."""
    rng = np.random.default_rng(2026)
    cuts = ge2 = ge3 = complemented = 0
    for k in range(3000):
        a, b, x = single_row(rng)
        r = ref.separate_row(a, b, x, np.zeros(NB), np.ones(NB), range(NB))
        if r['status'] not in (ref.CUT, ref.SHALLOW):
            continue
        feasible = POINTS @ a >= b
        assert feasible.any()
        assert np.all(POINTS[feasible] @ r['pi'] >= r['pi0']), (k, a, b, r['pi'], r['pi0'])
        if r['status'] == ref.CUT:
            assert r['pi0'] - float(r['pi'] @ x) > 0.0
            cuts += 1
            ge2 += bool(r['alpha'].max() >= 2)
            ge3 += bool(r['alpha'].max() >= 3)
            complemented += bool(np.any(r['pi'] > 0))
    print('cuts', cuts, 'coefficient >= 2:', ge2, '>= 3:', ge3, 'with a complemented column:', complemented)
    assert cuts >= 1000 and ge2 >= 50 and ge3 >= 1 and complemented >= 100


# ---- validity by HiGHS on rows that mix column kinds, inside a node's box ------------------------------------------

def mixed_model(seed):
    """8 binaries, 3 general integers in [0, 4], 3 continuous columns in [0, 2.5]; 4 rows of non-integer weights of
    both signs; a node's box that fixes two binaries."""
    rng = np.random.default_rng(100 + seed)
    n, m = 14, 4
    G = rng.integers(1, 30, (m, n)) / 7.0 * np.where(rng.random((m, n)) < 0.25, -1.0, 1.0)
    G *= rng.random((m, n)) < 0.8
    G[:, 8:] *= 0.125   # (relaxing a column out loosens the knapsack: with large coefficients there no cover is left)
    l = np.zeros(n)
    u = np.concatenate([np.ones(8), np.full(3, 4.0), np.full(3, 2.5)])
    lo = (np.minimum(G, 0.0) * u).sum(1)
    hi = (np.maximum(G, 0.0) * u).sum(1)
    d = lo + rng.uniform(0.3, 0.6, m) * (hi - lo)
    c = -rng.integers(1, 20, n).astype(np.float64)
    ln, un = l.copy(), u.copy()
    fixed = rng.choice(8, 2, replace=False)
    ln[fixed[0]] = 1.0   # fixed at 1
    un[fixed[1]] = 0.0   # fixed at 0
    return -G, -d, c, l, u, ln, un, list(range(11))


def test_cuts_of_mixed_rows_in_a_node_box_are_valid_by_highs():
    found = [mixed_cuts_checked(seed) for seed in range(8)]
    print('cuts', found)
    assert sum(found) >= 8, found


def mixed_cuts_checked(seed):
    A, b, c, l, u, ln, un, ints = mixed_model(seed)
    found = 0
    for box_l, box_u in ((l, u), (ln, un)):
        res = linprog(c, A_ub=-A, b_ub=-b, bounds=list(zip(box_l, box_u)), method='highs')
        if res.status != 0:
            continue
        out = ref.separate(A, b, res.x[None], box_l[None], box_u[None], ints)
        integrality = np.zeros(len(c))
        integrality[ints] = 1
        for i in np.flatnonzero(np.isin(out['status'][0], (ref.CUT, ref.SHALLOW))):
            pi, pi0 = out['pi'][0, i], out['pi0'][0, i]
            assert not pi[8:].any() and np.all(pi == np.round(pi)) and pi0 == round(pi0)
            assert not pi[box_l == box_u].any()   # (a fixed binary is no item)
            h = milp(pi, constraints=LinearConstraint(A, lb=b, ub=np.inf), bounds=Bounds(box_l, box_u),
                     integrality=integrality, options=dict(mip_rel_gap=0.0))
            assert h.status in (0, 2)
            if h.status == 0:   # (2: the node is infeasible, every cut is valid)
                assert float(h.fun) >= pi0 - 1e-6 * (abs(pi0) + float(np.abs(pi) @ box_u)), (seed, i, h.fun, pi0)
            found += int(out['status'][0, i] == ref.CUT)
    return found


# ---- the instance family and the root loop ------------------------------------------------------------------------

def test_the_sparse_knapsack_family():
    A, b, c, l, u, ints = sparse_knapsack_milp_arrays(40, 20, 8, seed=3)
    assert A.shape == (20, 40) and b.shape == (20,) and c.shape == (40,) and ints == list(range(40))
    assert np.all((A != 0).sum(1) == 8) and np.all(A <= 0) and np.all(A[A != 0] <= -5) and np.all(A >= -30)
    assert np.array_equal(b, -np.floor(0.5 * (-A).sum(1))) and np.all((c <= -5) & (c >= -30))
    assert np.array_equal(l, np.zeros(40)) and np.array_equal(u, np.ones(40))
    again = sparse_knapsack_milp_arrays(40, 20, 8, seed=3)
    assert all(np.array_equal(p, q) for p, q in zip((A, b, c), again[:3]))
    assert not np.array_equal(A, sparse_knapsack_milp_arrays(40, 20, 8, seed=4)[0])
    rng = np.random.Generator(np.random.PCG64(3))   # (the stream: one row after the other, then c)
    cols = rng.choice(40, size=8, replace=False)
    assert np.array_equal(np.sort(np.flatnonzero(A[0])), np.sort(cols))
    assert np.array_equal(-A[0, cols], rng.integers(5, 31, 8))


def test_general_integer_rows_have_no_cover():
    A, b, c, l, u, ints = random_dense_milp_arrays(20, 10, seed=1)
    x = linprog(c, A_ub=-A, b_ub=-b, bounds=list(zip(l, u)), method='highs').x
    out = ref.separate(A, b, x[None], l[None], u[None], ints)
    assert np.all(out['status'] == ref.NO_COVER) and not out['pi'].any() and not out['cover_size'].any()


class HighsRows:
    """One row set for root_cut_loop on the CPU: HiGHS for the LP (no basis: no tableau rows), the restatements for
    the two separations."""
    cover_calls = []

    def __init__(self, A, b, c):
        self.A, self.b, self.c = A, b, c

    def solve(self, l, u, vstat):
        res = linprog(self.c, A_ub=-self.A, b_ub=-self.b, bounds=list(zip(l, u)), method='highs')
        if res.status != 0:
            return dict(status=1, obj=INF, x=None, y=None, vstat=None, npivots=int(res.nit))
        m, n = self.A.shape
        return dict(status=0, obj=float(res.fun), x=res.x, y=-np.asarray(res.ineqlin.marginals),
                    vstat=np.zeros(n + m, np.int8), npivots=int(res.nit))

    def separate(self, x, l, u, int_idx, row_integral, multipliers, **params):
        out = mir_reference.separate(self.A, self.b, x[None], l[None], u[None], int_idx, row_integral, multipliers, **params)
        return dict(pi=out['pi'][0], pi0=out['pi0'][0], efficacy=out['efficacy'][0], status=out['status'][0])

    def separate_cover(self, x, l, u, int_idx, rows, min_efficacy):
        HighsRows.cover_calls.append((self.A.shape[0], None if rows is None else list(rows)))
        out = ref.separate(self.A, self.b, x[None], l[None], u[None], int_idx, rows, min_efficacy)
        return dict(pi=out['pi'][0], pi0=out['pi0'][0], efficacy=out['efficacy'][0], status=out['status'][0])


@pytest.mark.parametrize('seed', [0, 1])
def test_the_root_loop_with_covers_on_the_restatement(seed):
    """16 x 8 x 6: the first round finds violated covers on the model's rows (6 to 13 in the CPU prototype), the later
    rounds separate the model's rows only, the cuts kept are valid by HiGHS, and with cover=False the return value has
    the keys it had."""
    A, b, c, l, u, ints = sparse_knapsack_milp_arrays(16, 8, 6, seed=seed)
    HighsRows.cover_calls = []
    out = mir_cuts.root_cut_loop(A, b, c, l, u, ints, rounds=10, make_rows=HighsRows, cover=True)
    st, cs = out['stats'], out['cover_stats']
    print(seed, st, cs)
    assert list(cs) == ['rounds', 'rows', 'found', 'skipped', 'selected', 'kept', 'kernel_us']
    assert cs['rounds'] == st['rounds'] >= 1 and cs['rows'] == 8 * cs['rounds'] and cs['skipped'] == 0
    assert cs['found'] >= 6 and 1 <= cs['kept'] <= cs['selected'] <= cs['found']
    assert st['kept'] + cs['kept'] == len(out['cuts']) and st['kept'] <= st['selected'] <= st['found']
    assert st['bound_after'] > st['bound_before']
    assert HighsRows.cover_calls[0] == (8, None)
    assert all(rows == list(range(8)) for mk, rows in HighsRows.cover_calls if mk > 8) and len(HighsRows.cover_calls) == cs['rounds']
    for pi, pi0 in out['cuts']:
        h = milp(pi, constraints=LinearConstraint(A, lb=b, ub=np.inf), bounds=Bounds(l, u), integrality=np.ones(16),
                 options=dict(mip_rel_gap=0.0))
        assert h.status == 0 and float(h.fun) >= pi0 - 1e-6 * (abs(pi0) + float(np.abs(pi).sum()))
    # the gap the cover cuts close: well above what MIR closes on its best families (11 to 28 %)
    h = milp(c, constraints=LinearConstraint(A, lb=b, ub=np.inf), bounds=Bounds(l, u), integrality=np.ones(16),
             options=dict(mip_rel_gap=0.0))
    closed = (st['bound_after'] - st['bound_before']) / (float(h.fun) - st['bound_before'])
    print(seed, 'root gap closed', closed)
    assert closed >= 0.3
    off = mir_cuts.root_cut_loop(A, b, c, l, u, ints, rounds=3, make_rows=HighsRows)
    assert list(off) == ['cuts', 'A', 'b', 'vstat', 'stats']
    assert list(off['stats']) == ['rounds', 'base_rows', 'found', 'selected', 'kept', 'bound_before', 'bound_after',
                                  'lp_pivots', 'kernel_us']
