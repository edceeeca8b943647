"""The lifted cover separation on the GPU (include/mipx_cover.h): the kernel against the NumPy restatement
(tests/support/cover_reference.py), status and cover size exact and pi, pi0 and the efficacy bit for bit, at every
shape where the kernel's loops change their trip counts (one column; one wave of columns and one past it; one
workgroup and one past it; four columns per thread), on content chosen for each path, and the argument checks of
the entry."""
import functools

import numpy as np
import pytest

from simple_mip_solver_amd import MILPInstance, _ffi
from simple_mip_solver_amd.generators import random_dense_milp_arrays, sparse_knapsack_milp_arrays
from simple_mip_solver_amd.utils import cover_cuts
from tests.support import cover_reference as ref

pytestmark = pytest.mark.gpu
INF = float('inf')
COLUMNS = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024]
POINTS = 65


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


@functools.lru_cache(maxsize=None)
def instance(n, m, kind):
    """m knapsack rows over n columns.  'int': integer weights 1..30; 'real': weights that are no integers (they pin
    the order of every sum).  A quarter of the weights is negative; rows 0, 3, 6, ... are dense (up to four items per
    thread), the others keep about 12 nonzeros; from 8 columns on every eighth column is a general integer in [0, 4]
    and the one behind it continuous in [0, 2.5], both with small coefficients; the capacity is at 35 to 65 % of the
    reach.  65 points with many exact 0s and 1s."""
    rng = np.random.default_rng(1000 * n + 10 * m + (kind == 'real'))
    G = rng.integers(1, 31, (m, n)).astype(np.float64)
    if kind == 'real':
        G = G + rng.random((m, n)) * 0.75
    G *= np.where(rng.random((m, n)) < 0.25, -1.0, 1.0)
    keep = rng.random((m, n)) < min(1.0, 12.0 / n)
    keep[0::3] = True
    G *= keep
    u = np.ones(n)
    ints = np.ones(n, bool)
    if n >= 8:
        u[0::8], u[1::8] = 4.0, 2.5
        ints[1::8] = False
        G[:, 0::8] *= 0.125
        G[:, 1::8] *= 0.125
    l = np.zeros(n)
    lo, hi = (np.minimum(G, 0.0) * u).sum(1), (np.maximum(G, 0.0) * u).sum(1)
    d = lo + rng.uniform(0.35, 0.65, m) * (hi - lo)
    if kind == 'int':
        d = np.floor(d)
    X = rng.random((POINTS, n))
    where = rng.random((POINTS, n))
    X = np.where(where < 0.5, 1.0, np.where(where < 0.65, 0.0, X)) * u
    A, b = 0.0 - G, 0.0 - d
    for a in (A, b, l, u, X):
        a.setflags(write=False)
    return A, b, l, u, tuple(np.flatnonzero(ints).tolist()), X


def compare(ctx, n, m, kind, batch, rows, check_points, max_rows=12, min_efficacy=1e-6):
    A, b, l, u, ints, X = instance(n, m, kind)
    L, U = np.tile(l, (batch, 1)), np.tile(u, (batch, 1))
    p = _ffi.Problem(ctx, A, b, np.zeros(n))
    got = p.cover_separate_batch(X[:batch], L, U, ints, rows, min_efficacy)
    p.close()
    row_ids = list(range(m)) if rows is None else list(rows)
    R = len(row_ids)
    assert got['pi'].shape == (batch, R, n) and got['status'].shape == (batch, R) == got['cover_size'].shape
    assert np.all(np.isin(got['status'], (0, 1, 2, 4))) and got['kernel_us'] > 0
    check_points = [q for q in check_points if q < batch]
    sel = sorted(set(np.linspace(0, R - 1, min(R, max_rows)).astype(int).tolist()))
    exp = ref.separate(A, b, X[check_points], L[check_points], U[check_points], ints, [row_ids[k] for k in sel], min_efficacy)
    seen = set()
    for k, q in enumerate(check_points):
        for j, r in enumerate(sel):
            where = (n, m, kind, batch, q, row_ids[r])
            print(where, 'status', got['status'][q, r], exp['status'][k, j], 'size', got['cover_size'][q, r],
                  'efficacy', got['efficacy'][q, r], 'largest coefficient', np.abs(got['pi'][q, r]).max())
            assert got['status'][q, r] == exp['status'][k, j], where
            assert got['cover_size'][q, r] == exp['cover_size'][k, j], where
            assert np.array_equal(bits(got['pi'][q, r]), bits(exp['pi'][k, j])), where
            assert bits(got['pi0'][q, r]) == bits(exp['pi0'][k, j]), where
            assert bits(got['efficacy'][q, r]) == bits(exp['efficacy'][k, j]), where
            seen.add(int(exp['status'][k, j]))
    # rows that were not compared: what must hold of any output
    none = np.isin(got['status'], (ref.NO_COVER, ref.SKIPPED))
    assert not got['pi'][none].any() and not got['pi0'][none].any() and not got['cover_size'][none].any()
    assert np.all(got['cover_size'][~none] >= 1) and np.all(got['pi'] == np.round(got['pi']))
    return got, seen


@pytest.mark.parametrize('kind', ['int', 'real'])
@pytest.mark.parametrize('n', COLUMNS)
def test_three_rows_equal_the_restatement(n, kind, gpu_ctx):
    """m = 3 (a dense row and two sparse ones), batch 3, every row of every point compared."""
    compare(gpu_ctx, n, 3, kind, 3, None, [0, 1, 2])


@pytest.mark.parametrize('n', COLUMNS)
def test_one_row_and_one_point_equal_the_restatement(n, gpu_ctx):
    compare(gpu_ctx, n, 1, 'real', 1, None, [0])


@pytest.mark.parametrize('n', [2, 65, 257, 1024])
def test_130_rows_and_a_subset_equal_the_restatement(n, gpu_ctx):
    """m = 130: rows NULL, and a subset in an order of its own (the output follows the subset's order)."""
    compare(gpu_ctx, n, 130, 'real', 3, None, [0, 2], max_rows=10)
    subset = [129, 0, 64, 3, 77]
    got, _ = compare(gpu_ctx, n, 130, 'int', 3, subset, [0, 1, 2])
    A, b, l, u, ints, X = instance(n, 130, 'int')
    p = _ffi.Problem(gpu_ctx, A, b, np.zeros(n))
    full = p.cover_separate_batch(X[:3], np.tile(l, (3, 1)), np.tile(u, (3, 1)), ints)
    p.close()
    for key in ('pi', 'pi0', 'efficacy', 'cover_size', 'status'):
        assert np.array_equal(got[key], full[key][:, subset]), key


@pytest.mark.parametrize('n', [1, 64, 256, 1023])
def test_a_batch_of_65_equals_the_restatement(n, gpu_ctx):
    compare(gpu_ctx, n, 3, 'real', 65, None, [0, 31, 63, 64])
    compare(gpu_ctx, n, 130, 'int', 65, [5, 128], [1, 64])


def test_cuts_and_lifted_coefficients_occur(gpu_ctx):
    """The instances are not tame: cuts, shallow rows and rows without a cover occur, and coefficients of 2 and more."""
    seen, largest = set(), 0.0
    for n in (65, 257):
        got, _ = compare(gpu_ctx, n, 130, 'int', 65, None, [0], max_rows=4)
        seen |= set(got['status'].ravel().tolist())
        largest = max(largest, float(np.abs(got['pi'][got['status'] == 0]).max()))
    assert {ref.CUT, ref.NO_COVER, ref.SHALLOW} <= seen and largest >= 2.0, (seen, largest)


def one_row(ctx, a, b, x, l, u, ints, status, min_efficacy=1e-6):
    """One row on the GPU against the restatement and the status the case is there for (None: any)."""
    a, x, l, u = (np.asarray(v, np.float64) for v in (a, x, l, u))
    p = _ffi.Problem(ctx, a[None], np.array([float(b)]), np.zeros(len(a)))
    got = p.cover_separate_batch(x[None], l[None], u[None], list(ints), None, min_efficacy)
    p.close()
    exp = ref.separate_row(a, b, x, l, u, list(ints), min_efficacy)
    print('status', got['status'][0, 0], exp['status'], 'size', got['cover_size'][0, 0], 'efficacy', got['efficacy'][0, 0])
    assert exp['status'] == got['status'][0, 0] and status in (None, exp['status'])
    assert got['cover_size'][0, 0] == exp['cover_size']
    assert np.array_equal(bits(got['pi'][0, 0]), bits(exp['pi'])) and bits(got['pi0'][0, 0]) == bits(exp['pi0'])
    assert bits(got['efficacy'][0, 0]) == bits(exp['efficacy'])
    return exp


@pytest.mark.parametrize('n', [5, 65, 257, 1024])
def test_the_content_cases(n, gpu_ctx):
    rng = np.random.default_rng(n)
    zeros, ones, every = np.zeros(n), np.ones(n), range(n)
    sign = np.where(np.arange(n) % 3 == 2, -1.0, 1.0)
    at_one = np.where(sign < 0, 0.0, 1.0)   # the point at which every y* = 1
    cap = lambda g, share: (np.minimum(g, 0.0).sum() + share * np.abs(g).sum())   # W = share of the weights
    wi = rng.integers(1, 31, n) * sign
    wr = (rng.integers(1, 31, n) + rng.random(n) * 0.75) * sign
    x = np.where(sign < 0, 1.0 - 0.9 * rng.random(n) ** 4, 0.9 * rng.random(n) ** 4 + 0.1)
    near_one = np.where(sign < 0, 0.5 / n, 1.0 - 0.5 / n)   # every y* = 1 - 0.5 / n: a cover of r items is violated by 1 - 0.5 r / n
    # integer and non-integer weights at a fractional point
    one_row(gpu_ctx, -wi, -np.floor(cap(wi, 0.5)), near_one, zeros, ones, every, ref.CUT)
    one_row(gpu_ctx, -wr, -cap(wr, 0.5), near_one, zeros, ones, every, ref.CUT)
    one_row(gpu_ctx, -wr, -cap(wr, 0.3), x, zeros, ones, every, None)
    # exact ties in ratio and in weight: the index decides both orders
    e = one_row(gpu_ctx, -2.0 * sign, -cap(2.0 * sign, 0.5) - 1.0, near_one, zeros, ones, every, ref.CUT)
    assert e['cover'].tolist() == list(range(e['cover_size']))   # (C0 is a run of the lowest numbers, and all of it is needed)
    tied = np.where(np.arange(n) % 2 == 0, 3.0, 6.0) * sign   # two weights, the ratios tied inside each
    one_row(gpu_ctx, -tied, -np.floor(cap(tied, 0.4)), np.full(n, 0.5), zeros, ones, every, None)
    one_row(gpu_ctx, -tied, -np.floor(cap(tied, 0.4)), at_one, zeros, ones, every, ref.CUT)
    # every y* = 1 (violated by one at the least), every y* = 0 (nothing is violated)
    e = one_row(gpu_ctx, -wi, -np.floor(cap(wi, 0.5)), at_one, zeros, ones, every, ref.CUT)
    assert e['pi0'] - float(e['pi'] @ at_one) >= 1.0
    one_row(gpu_ctx, -wi, -np.floor(cap(wi, 0.5)), 1.0 - at_one, zeros, ones, every, ref.SHALLOW)
    # x* slightly outside its box: y* is clipped for the order, the efficacy takes the point as it is
    out = at_one + np.where(np.arange(n) % 2 == 0, 1e-9, -1e-9)
    one_row(gpu_ctx, -wr, -cap(wr, 0.5), out, zeros, ones, every, ref.CUT)
    # no cover: the whole row fits; fewer than two binaries
    one_row(gpu_ctx, -wr, -cap(wr, 1.0), at_one, zeros, ones, every, ref.NO_COVER)
    one_row(gpu_ctx, -wi, -np.floor(cap(wi, 0.5)), at_one, zeros, ones, [0], ref.NO_COVER)
    # skipped: a column that is no binary needs its infinite upper bound; a negative capacity
    uinf = ones.copy()
    uinf[2] = INF   # (column 2 has a negative weight: it is relaxed out at u)
    one_row(gpu_ctx, -wi, -np.floor(cap(wi, 0.5)), at_one, zeros, uinf, every, ref.SKIPPED)
    uinf = ones.copy()
    uinf[0] = INF   # (column 0 has a positive weight: it is relaxed out at l, the bound is not needed)
    one_row(gpu_ctx, -wi, -np.floor(cap(wi[1:], 0.5)), at_one, zeros, uinf, every, ref.CUT)
    one_row(gpu_ctx, -wi, -(np.minimum(wi, 0.0).sum() - 1.0), at_one, zeros, ones, every, ref.SKIPPED)
    # shallow by the threshold alone
    e = one_row(gpu_ctx, -wi, -np.floor(cap(wi, 0.5)), near_one, zeros, ones, every, ref.SHALLOW,
                min_efficacy=10.0)
    assert e['pi'].any() and e['cover_size'] >= 1 and 1e-6 < e['efficacy'] <= 10.0
    # a cover of size n: unit weights, a capacity half a unit short of all of them
    e = one_row(gpu_ctx, -sign, -(np.minimum(sign, 0.0).sum() + n - 0.5), at_one, zeros, ones, every, ref.CUT)
    assert e['cover_size'] == n and np.all(np.abs(e['pi']) == 1.0)
    # shifted boxes, a fixed binary and a general integer among the items
    l2, u2 = zeros + 2.0, ones + 2.0
    u2[1], u2[3] = 2.0, 7.0
    shift = wr @ np.where(sign < 0, u2, l2)   # (what relaxing and shifting take from the right-hand side)
    e = one_row(gpu_ctx, -wr, -(0.5 * np.abs(np.delete(wr, [1, 3])).sum() + shift), at_one + 2.0, l2, u2, every, ref.CUT)
    assert not e['pi'][[1, 3]].any()


def test_separate_covers_and_the_argument_errors(gpu_ctx):
    A, b, c, l, u, ints = sparse_knapsack_milp_arrays(16, 8, 6, seed=0)
    model = MILPInstance(A=A.copy(), b=b.copy(), c=c.copy(), l=l.copy(), u=u.copy(), integerIndices=list(ints),
                         sense=['Min', '>='], numVars=16)
    p = _ffi.Problem(gpu_ctx, A, b, c)
    X = np.vstack([p.solve_batch(l[None], u[None])['x'], np.full((2, 16), 0.5)])
    X[2, ::2] = 1.0
    pi, pi0, eff, size, status = cover_cuts.separate_covers(model, X)
    exp = ref.separate(A, b, X, np.tile(l, (3, 1)), np.tile(u, (3, 1)), ints)
    assert pi.shape == (3, 8, 16) and np.array_equal(status, exp['status']) and np.array_equal(size, exp['cover_size'])
    assert np.array_equal(bits(pi), bits(exp['pi'])) and np.array_equal(bits(pi0), bits(exp['pi0']))
    assert np.array_equal(bits(eff), bits(exp['efficacy']))
    assert int(np.sum(status[0] == 0)) >= 6   # (the root LP point: 6 to 13 violated covers in the CPU prototype)
    # a node's box: two columns fixed are no items any more
    L, U = np.tile(l, (3, 1)), np.tile(u, (3, 1))
    fixed = np.flatnonzero(A[0])[:2]
    L[:, fixed[0]] = 1.0
    U[:, fixed[1]] = 0.0
    out = cover_cuts.separate_covers(model, np.clip(X, L, U), L=L, U=U, rows=[0, 5])
    exp = ref.separate(A, b, np.clip(X, L, U), L, U, ints, [0, 5])
    assert out[0].shape == (3, 2, 16) and np.array_equal(bits(out[0]), bits(exp['pi'])) and not out[0][:, :, fixed].any()
    assert np.array_equal(out[4], exp['status'])
    one = cover_cuts.separate_covers(model, X[0])
    assert one[0].shape == (1, 8, 16) and np.array_equal(one[4][0], status[0])
    # general integers: no row has a cover
    Ad, bd, cd, ld, ud, intsd = random_dense_milp_arrays(20, 10, seed=1)
    pd = _ffi.Problem(gpu_ctx, Ad, bd, cd)
    xd = pd.solve_batch(ld[None], ud[None])['x']
    got = pd.cover_separate_batch(xd, ld[None], ud[None], intsd)
    pd.close()
    assert np.all(got['status'] == ref.NO_COVER) and not got['pi'].any()
    with pytest.raises(AssertionError, match='one point of n columns'):
        cover_cuts.separate_covers(model, X[:, :5])
    with pytest.raises(AssertionError, match='one box per point'):
        cover_cuts.separate_covers(model, X, L=np.zeros((2, 16)), U=np.ones((2, 16)))
    with pytest.raises(AssertionError, match='list of row indices'):
        cover_cuts.separate_covers(model, X, rows=[0.5])
    with pytest.raises(AssertionError, match='BranchAndBound or a MILPInstance'):
        cover_cuts.separate_covers(object(), X)
    Xbad = X.copy()
    Xbad[1, 4] = np.nan
    lbad, ubad, uninf = np.tile(l, (3, 1)), np.tile(u, (3, 1)), np.tile(u, (3, 1))
    lbad[0, 0], ubad[2, 3], uninf[1, 1] = -INF, np.nan, -INF
    for bad in (dict(x=Xbad), dict(l=lbad), dict(u=ubad), dict(u=uninf), dict(integer_indices=[0, 0, 1]),
                dict(integer_indices=[16]), dict(integer_indices=[-1]), dict(rows=[0, 0]), dict(rows=[8]), dict(rows=[-1]),
                dict(rows=[]), dict(min_efficacy=float('nan'))):
        kw = dict(x=X, l=np.tile(l, (3, 1)), u=np.tile(u, (3, 1)), integer_indices=list(ints))
        kw.update(bad)
        with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL'):
            p.cover_separate_batch(**kw)
    empty = p.cover_separate_batch(np.zeros((0, 16)), np.zeros((0, 16)), np.zeros((0, 16)), list(ints))
    assert empty['pi'].shape == (0, 8, 16) and empty['kernel_us'] == 0.0
    p.close()
