"""The MIR separation on the GPU (include/mipx_mir.h): the kernel against the NumPy restatement
(tests/support/mir_reference.py), status, sign and divisor exact and pi, pi0 and the efficacy bit for bit, at every
shape where the kernel's loops change their trip counts, and the argument checks of separate_mir."""
import functools

import numpy as np
import pytest

from simple_mip_solver_amd import MILPInstance, _ffi
from simple_mip_solver_amd.generators import random_dense_milp_arrays
from simple_mip_solver_amd.utils import mir_cuts
from tests.support import mir_reference as ref

pytestmark = pytest.mark.gpu
INF = float('inf')
# (n, m): smallest; generator size; one full wave of extended columns and one past it; one full workgroup and one
# past it; several columns per thread; near the limit
SHAPES = [(5, 3), (12, 6), (60, 4), (61, 4), (200, 56), (200, 57), (300, 150), (1000, 700)]
LP_SHAPES = SHAPES[:7]   # the shapes whose first point is the LP optimum (the last one's LP takes too long for a test)
POINTS = 65


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


@functools.lru_cache(maxsize=None)
def instance(n, m, variant):
    """'plain': the generator's instance; 'inf': every third column without an upper bound; 'cont': the odd columns
    continuous and the data divided by 7."""
    A, b, c, l, u, ints = random_dense_milp_arrays(n, m, seed=1)
    if variant == 'inf':
        u = u.copy()
        u[1::3] = INF
    if variant == 'cont':
        A, b, ints = A / 7.0, b / 7.0, list(range(0, n, 2))
    for a in (A, b, c, l, u):
        a.setflags(write=False)
    return A, b, c, l, u, tuple(ints)


@functools.lru_cache(maxsize=None)
def points(n, m, variant):
    """65 points: the LP optimum (or a random point at the largest shape), a random interior point, a point on its
    bounds, then random interior points; with the basis of the LP where it was solved."""
    A, b, c, l, u, ints = instance(n, m, variant)
    rng = np.random.default_rng(7 * n + m)
    top = np.where(np.isinf(u), l + 10.0, u)
    X = l + rng.random((POINTS, n)) * (top - l)
    X[2] = np.where(np.arange(n) % 2 == 0, l, top)
    vstat = None
    if (n, m) in LP_SHAPES:
        p = _ffi.Problem(_ffi.default_context(), A, b, c)
        res = p.solve_batch(l[None], u[None])
        p.close()
        if res['status'][0] == 0:
            X[0], vstat = res['x'][0], res['vstat'][0]
    X.setflags(write=False)
    return X, vstat


def multipliers(n, m, variant, rows):
    """None, or `rows` base rows: random sparse integer weights with negative entries, one dense real row, and the
    rows of B^-1 of the LP's basis where there is one."""
    if rows is None:
        return None
    A, b, c, l, u, ints = instance(n, m, variant)
    X, vstat = points(n, m, variant)
    rng = np.random.default_rng(11 * n + m + rows)
    M = rng.integers(-3, 4, (rows, m)).astype(np.float64) * (rng.random((rows, m)) < min(1.0, 4.0 / m))
    M[0] = rng.normal(size=m)
    if vstat is not None and rows > 1:
        T = mir_cuts.tableau_multipliers((A, b), vstat, X[0], ints, max_rows=rows - 1)
        M[1:1 + len(T)] = T
    return M


def compare(ctx, n, m, variant, rows, batch, check_points, max_checked=40, **params):
    A, b, c, l, u, ints = instance(n, m, variant)
    X, _ = points(n, m, variant)
    M = multipliers(n, m, variant, rows)
    flags = mir_cuts.row_integral_flags(A, b, ints)
    L, U = np.tile(l, (batch, 1)), np.tile(u, (batch, 1))
    p = _ffi.Problem(ctx, A, b, c)
    got = p.mir_separate_batch(X[:batch], L, U, ints, flags, M, **params)
    p.close()
    R = m if M is None else len(M)
    assert got['pi'].shape == (batch, R, n) and got['status'].shape == (batch, R)
    assert np.all((got['status'] >= 0) & (got['status'] <= 4)) and got['kernel_us'] > 0
    check_points = [q for q in check_points if q < batch]
    per_point = max(1, max_checked // len(check_points))
    sel = sorted(set(np.linspace(0, R - 1, min(R, per_point)).astype(int).tolist()))
    exp = ref.separate(A, b, X[check_points], L[check_points], U[check_points], ints, flags, M, rows=sel, **params)
    seen = set()
    for k, q in enumerate(check_points):
        for r in sel:
            where = (n, m, variant, rows, q, r)
            print(where, 'status', got['status'][q, r], exp['status'][k, r], 'sign', got['sign'][q, r], 'delta',
                  got['delta'][q, r], exp['index'][k, r], 'efficacy', got['efficacy'][q, r])
            assert got['status'][q, r] == exp['status'][k, r], where
            assert got['sign'][q, r] == exp['sign'][k, r], where
            assert bits(got['delta'][q, r]) == bits(exp['delta'][k, r]), where   # (the same entry of the same list)
            assert np.array_equal(bits(got['pi'][q, r]), bits(exp['pi'][k, r])), where
            assert bits(got['pi0'][q, r]) == bits(exp['pi0'][k, r]), where
            assert bits(got['efficacy'][q, r]) == bits(exp['efficacy'][k, r]), where
            seen.add(int(exp['status'][k, r]))
    return got, seen


@pytest.mark.parametrize('n,m', SHAPES)
def test_unit_rows_equal_the_restatement(n, m, gpu_ctx):
    """NULL multipliers, batch 3: the LP optimum, an interior point and a point on its bounds, which gives no trial on
    integer data (every divisor is 1.0 or a slack's, and d' is an integer)."""
    got, seen = compare(gpu_ctx, n, m, 'plain', None, 3, [0, 1, 2])
    assert np.all(got['status'][2] == ref.NO_TRIAL)


@pytest.mark.parametrize('variant', ['inf', 'cont'])
@pytest.mark.parametrize('n,m', SHAPES)
def test_dense_rows_equal_the_restatement(n, m, variant, gpu_ctx):
    """7 dense base rows (negative weights, a real row, rows of B^-1), batch 3, with columns without an upper bound
    and with half the columns continuous."""
    compare(gpu_ctx, n, m, variant, 7, 3, [0, 1, 2])


@pytest.mark.parametrize('n,m', SHAPES)
def test_one_row_and_many_rows_equal_the_restatement(n, m, gpu_ctx):
    compare(gpu_ctx, n, m, 'plain', 1, 1, [0])
    compare(gpu_ctx, n, m, 'inf', m + 3, 1, [0], max_checked=24)


@pytest.mark.parametrize('n,m', SHAPES[:4])
def test_a_batch_of_65_equals_the_restatement(n, m, gpu_ctx):
    compare(gpu_ctx, n, m, 'plain', None, 65, [0, 2, 31, 63, 64], max_checked=20)
    compare(gpu_ctx, n, m, 'cont', 7, 65, [1, 64], max_checked=14)


def test_the_statuses_all_occur_at_the_generator_size(gpu_ctx):
    """Over the unit rows and 7 dense rows at 12 x 6 the kernel returns cuts and rows without a trial."""
    seen = set()
    for rows in (None, 7):
        got, _ = compare(gpu_ctx, 12, 6, 'plain', rows, 65, [0, 1, 2], max_checked=39)
        seen |= set(got['status'].ravel().tolist())
    assert {ref.CUT, ref.NO_TRIAL} <= seen, seen


def test_the_hand_example_and_the_status_cases_on_the_gpu(gpu_ctx):
    cases = [([[-2.0, -2.0]], [-3.0], [0.75, 0.75], [0.0, 0.0], [1.0, 1.0], [0, 1], [1], ref.CUT),
             ([[-2.0, -2.0]], [-3.0], [1.0, 0.0], [0.0, 0.0], [1.0, 1.0], [0, 1], [1], ref.NO_TRIAL),
             ([[-2.0, -2.0]], [-3.0], [0.25, 0.25], [0.0, 0.0], [1.0, 1.0], [0, 1], [1], ref.SHALLOW),
             ([[-1.0, 1e-7]], [-0.5], [0.5, 0.0], [0.0, 0.0], [2.0, INF], [0], [0], ref.DYNAMISM),
             ([[-2.0, -2.0]], [-3.0], [0.75, 1.2], [0.0, 0.0], [1.0, 1.5], [0, 1], [1], ref.SKIPPED)]
    for A, b, x, l, u, ints, flags, status in cases:
        p = _ffi.Problem(gpu_ctx, np.array(A), np.array(b), np.zeros(2))
        got = p.mir_separate_batch(np.array([x]), np.array([l]), np.array([u]), ints, flags)
        p.close()
        exp = ref.separate_row(A, b, x, l, u, ints, flags, [1.0])
        assert exp['status'] == status == got['status'][0, 0], (x, got['status'])
        assert got['sign'][0, 0] == exp['sign'] and bits(got['delta'][0, 0]) == bits(exp['delta'])
        assert np.array_equal(bits(got['pi'][0, 0]), bits(exp['pi'])) and bits(got['pi0'][0, 0]) == bits(exp['pi0'])
        assert bits(got['efficacy'][0, 0]) == bits(exp['efficacy'])
    p = _ffi.Problem(gpu_ctx, np.array([[-2.0, -2.0]]), np.array([-3.0]), np.zeros(2))
    got = p.mir_separate_batch([[0.75, 0.75]], [[0.0, 0.0]], [[1.0, 1.0]], [0, 1], [1])
    p.close()
    assert np.array_equal(got['pi'][0, 0], [-1.0, -1.0]) and got['pi0'][0, 0] == -1.0
    assert got['delta'][0, 0] == 2.0 and got['sign'][0, 0] == 1 and got['status'][0, 0] == 0


def test_a_row_with_more_than_16_divisors_and_a_row_outside_the_window(gpu_ctx):
    """A real-valued base row over 60 columns has more distinct |g| than the list takes: the list is the first 16 in
    column order, then 1.0.  On the integer rows at an interior point d' is an integer: the trial at 1.0 is refused by
    the window, and the restatement and the kernel agree on what is left."""
    A, b, c, l, u, ints = instance(60, 4, 'plain')
    X, _ = points(60, 4, 'plain')
    M = multipliers(60, 4, 'plain', 1)
    flags = mir_cuts.row_integral_flags(A, b, ints)
    one = ref.separate_row(A, b, X[1], l, u, ints, flags, M[0])
    assert len(one['candidates']) == 17 and one['candidates'][-1] == 1.0 and len(set(one['candidates'])) == 17
    for divisors in (16, 3, 64):
        compare(gpu_ctx, 60, 4, 'plain', 1, 3, [0, 1], max_divisors=divisors)
    unit = ref.separate_row(A, b, X[1], l, u, ints, flags, np.eye(4)[0], f0_min=0.3)
    assert unit['index'] is None or unit['candidates'][unit['index'][0]] != 1.0 or unit['index'][1] > 0
    compare(gpu_ctx, 60, 4, 'plain', None, 3, [0, 1, 2], f0_min=0.3)
    compare(gpu_ctx, 60, 4, 'cont', 7, 3, [0, 1, 2], f0_min=0.3, max_dynamism=50.0, min_efficacy=0.05)


def test_separate_mir_and_its_argument_errors(gpu_ctx):
    A, b, c, l, u, ints = instance(12, 6, 'plain')
    X, vstat = points(12, 6, 'plain')
    model = MILPInstance(A=A.copy(), b=b.copy(), c=c.copy(), l=l.copy(), u=u.copy(), integerIndices=list(ints),
                         sense=['Min', '>='], numVars=12)
    pi, pi0, eff, delta, sign, status = mir_cuts.separate_mir(model, X[:3])
    exp = ref.separate(A, b, X[:3], np.tile(l, (3, 1)), np.tile(u, (3, 1)), ints, mir_cuts.row_integral_flags(A, b, ints))
    assert pi.shape == (3, 6, 12) and np.array_equal(status, exp['status'])
    assert np.array_equal(bits(pi), bits(exp['pi'])) and np.array_equal(bits(pi0), bits(exp['pi0']))
    T = mir_cuts.tableau_multipliers((A, b), vstat, X[0], ints)
    assert len(T) >= 1
    out = mir_cuts.separate_mir(model, X[0], multipliers=T)
    assert out[0].shape == (1, len(T), 12)
    with pytest.raises(AssertionError, match='one point of n columns'):
        mir_cuts.separate_mir(model, X[:3, :5])
    with pytest.raises(AssertionError, match='one box per point'):
        mir_cuts.separate_mir(model, X[:3], L=np.zeros((2, 12)), U=np.ones((2, 12)))
    with pytest.raises(AssertionError, match=r'\(R, m\) matrix'):
        mir_cuts.separate_mir(model, X[:3], multipliers=np.ones((2, 5)))
    with pytest.raises(AssertionError, match='parameters are'):
        mir_cuts.separate_mir(model, X[:3], depth=3)
    with pytest.raises(AssertionError, match='BranchAndBound or a MILPInstance'):
        mir_cuts.separate_mir(object(), X[:3])
    for bad in (dict(f0_min=0.0), dict(f0_min=0.5), dict(max_divisors=0), dict(max_divisors=65), dict(max_dynamism=0.5),
                dict(min_efficacy=float('nan'))):
        with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL'):
            mir_cuts.separate_mir(model, X[:3], **bad)
    Xbad = X[:3].copy()
    Xbad[1, 4] = np.nan
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL'):
        mir_cuts.separate_mir(model, Xbad)
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL'):
        mir_cuts.separate_mir(model, X[:3], multipliers=np.full((2, 6), np.inf))
    p = _ffi.Problem(gpu_ctx, A, b, c)
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL'):
        p.mir_separate_batch(X[:1], l[None], u[None], [0, 0, 1])
    with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL'):
        p.mir_separate_batch(X[:1], np.full((1, 12), -INF), u[None], list(ints))
    p.close()
