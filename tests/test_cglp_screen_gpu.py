"""The dual screen of the support sessions on the GPU (include/mipx_cglp_screen.h): support_screen and the pack kernels
against the NumPy restatement bit for bit (tests/support/cglp_screen_reference.py), a screening session against HiGHS
and against a session without the options, the separator with screen and in-out on the 101-leaf tree whose extended
formulation HiGHS solves, and that asking for the cold retry changes nothing where no leaf fails.  No session here
has a leaf LP that fails, so the retry's own path (the packing by verdict, the cold gather, the scatter of a failed LP
and of a second LP) is NOT covered here: tests/test_support_kernels_gpu.py runs it on synthetic leaves."""
import numpy as np
import pytest

from simple_mip_solver_amd import BaseNode, BranchAndBound, DisjunctiveSeparator, PseudoCostBranchNode, _ffi
from simple_mip_solver_amd.generators import random_dense_milp_arrays
from tests.support import cglp_reference as highs
from tests.support import cglp_screen_reference as ref
from tests.test_cglp_separation_gpu import (HIGHS_TOL, M, N, SEED, childless_not_infeasible, generator_model, highs_optimum,
                                            scale_of)

pytestmark = pytest.mark.gpu
SIZES = (1, 63, 64, 65, 2047, 2048, 2049)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


# ---- the kernels on a caller's data ------------------------------------------------------------------------------
def synthetic(m, n, T, rng):
    """Leaves as the screen may meet them: sparse duals with negative and zero entries, some leaves without duals."""
    l = rng.uniform(-3, 3, (T, n)).round(2)
    u = l + rng.uniform(0, 4, (T, n)).round(2)          # (some columns fixed: width 0)
    y = rng.uniform(-0.5, 2.0, (T, m)) * (rng.random((T, m)) < 0.4)
    has_y = (rng.random(T) < 0.85).astype(np.uint8)
    return l, u, y, has_y


def check_batch(p, A, b, pi, pi0, screen_tol, l, u, y, has_y, what):
    want = ref.screen(A, b, pi, pi0, screen_tol, l, u, y, has_y)
    got = p.support_screen_batch(pi, pi0, screen_tol, l, u, y, has_y)
    assert np.array_equal(got['bound'], want['bound'], equal_nan=True), what
    finite = np.isfinite(want['bound'])
    assert np.array_equal(bits(got['bound'][finite]), bits(want['bound'][finite])), what
    assert np.array_equal(got['screened'], want['screened']), what
    assert got['count'] == want['count'] and np.array_equal(got['packed'], want['packed']), what
    return want


@pytest.mark.parametrize('m, n', [(1, 1), (3, 5), (20, 40), (64, 64), (65, 129)])
def test_screen_and_pack_match_the_restatement_bit_for_bit(gpu_ctx, m, n):
    rng = np.random.default_rng(1000 * m + n)
    A, b, c = rng.standard_normal((m, n)), rng.standard_normal(m), np.zeros(n)
    p = _ffi.Problem(gpu_ctx, A, b, c)
    try:
        for T in SIZES:
            pi = rng.uniform(-1, 1, n)
            l, u, y, has_y = synthetic(m, n, T, rng)
            L = ref.bound(A, b, pi, l, u, y, has_y)
            assert np.all(np.isfinite(L[has_y != 0]))
            pi0 = float(np.median(L[has_y != 0])) if has_y.any() else 0.0     # about half of them screen
            want = check_batch(p, A, b, pi, pi0, 1e-7, l, u, y, has_y, (m, n, T))
            if T >= 63:
                assert 0 < want['count'] < T and 0.25 * T < want['screened'].sum() < 0.6 * T
    finally:
        p.close()


def test_screen_all_none_and_values_that_are_not_finite(gpu_ctx):
    m, n, T = 20, 40, 2049
    rng = np.random.default_rng(7)
    A, b = rng.standard_normal((m, n)), rng.standard_normal(m)
    p = _ffi.Problem(gpu_ctx, A, b, np.zeros(n))
    try:
        pi = rng.uniform(-1, 1, n)
        l, u, y, _ = synthetic(m, n, T, rng)
        ones = np.ones(T, np.uint8)
        L = ref.bound(A, b, pi, l, u, y, ones)
        everyone = check_batch(p, A, b, pi, float(L.min()) - 1.0, 0.0, l, u, y, ones, 'all screened')
        assert everyone['count'] == 0 and np.all(everyone['packed'] == -1) and everyone['screened'].all()
        nobody = check_batch(p, A, b, pi, float(L.max()) + 1.0, 0.5, l, u, y, ones, 'none screened')
        assert nobody['count'] == T and np.array_equal(nobody['packed'], np.arange(T))
        without = check_batch(p, A, b, pi, float(L.min()) - 1.0, 0.0, l, u, y, np.zeros(T, np.uint8), 'no duals on record')
        assert without['count'] == T and np.all(without['bound'] == -np.inf)
        # the margin exactly at -screen_tol screens, an ulp below does not
        k = int(np.argsort(L)[T // 2])
        at = check_batch(p, A, b, pi, float(L[k]), 0.0, l, u, y, ones, 'at the tolerance')
        assert at['screened'][k] == 1
        below = check_batch(p, A, b, pi, float(np.nextafter(L[k], np.inf)), 0.0, l, u, y, ones, 'an ulp below')
        assert below['screened'][k] == 0
        # a NaN dual reads as 0; an infinite one gives a bound that is not finite, which never screens
        y[5, 3], y[6, 2], y[7, 1] = np.nan, np.inf, -np.inf
        odd = check_batch(p, A, b, pi, -1e300, 0.0, l, u, y, ones, 'not finite')
        assert odd['screened'][5] == 1 and odd['screened'][6] == 0 and odd['screened'][7] == 1
        assert odd['packed'][:odd['count']].tolist() == [6]
    finally:
        p.close()


def test_batch_entry_refusals(gpu_ctx):
    A, b = np.ones((2, 3)), np.ones(2)
    p = _ffi.Problem(gpu_ctx, A, b, np.zeros(3))
    l, u, y, has_y = np.zeros((4, 3)), np.ones((4, 3)), np.zeros((4, 2)), np.ones(4, np.uint8)
    with pytest.raises(_ffi.MipxError, match='bad argument'):
        p.support_screen_batch(np.zeros(3), 0.0, -1.0, l, u, y, has_y)
    with pytest.raises(_ffi.MipxError, match='bad argument'):
        p.support_screen_batch(np.zeros(3), np.nan, 0.0, l, u, y, has_y)
    out = p.support_screen_batch(np.zeros(3), 0.0, 0.0, l[:0], u[:0], y[:0], has_y[:0])
    assert out['count'] == 0 and len(out['bound']) == 0
    p.close()   # (MIPX_ETOOBIG cannot be reached from here: no problem above 1024 rows or columns can be made)


# ---- a session ---------------------------------------------------------------------------------------------------
_cache = {}


def tree():
    """40 x 20 in batches of 256: a few hundred not-infeasible childless nodes."""
    if 'bb' not in _cache:
        bb = BranchAndBound(generator_model(N, M, SEED), PseudoCostBranchNode, pseudo_costs={}, gomory_cuts=False,
                            frontier_batch=256, tree_record=True, mip_gap=0.0, node_limit=700)
        bb.solve()
        _cache['bb'] = bb
    return _cache['bb']


def directions():
    """Three directions in a row, close to one another as a master's are, and a right-hand side in the middle of the
    first one's support values (so that later evaluations screen some leaves and solve others)."""
    if 'dirs' not in _cache:
        bb = tree()
        ids = childless_not_infeasible(bb)
        rng = np.random.default_rng(5)
        base = rng.uniform(-1, 1, N)
        pis = [np.clip(base + 0.02 * k * rng.uniform(-1, 1, N), -1, 1) for k in range(3)]
        A, b, _, _, _, _ = random_dense_milp_arrays(N, M, seed=SEED)
        ses = bb._native.support_open(ids)
        first = ses.eval(pis[0], 0.0, want_margins=True)
        live = ses.leaves()
        ses.close()
        pi0 = float(np.quantile(first['margins'], 0.4))
        Lb, Ub = bb._native.node_bounds(live)
        H = np.array([[highs.support(pi, A, b, Lb[k], Ub[k])[1] for k in range(len(live))] for pi in pis])   # HiGHS, once
        _cache['dirs'] = (ids, live, pis, pi0, H)
    return _cache['dirs']


def same(a, b):
    assert sorted(a) == sorted(b)
    for key in a:
        if isinstance(a[key], np.ndarray) and a[key].dtype == np.float64:
            assert np.array_equal(bits(a[key]), bits(b[key])), key
        elif isinstance(a[key], np.ndarray):
            assert np.array_equal(a[key], b[key]), key
        else:
            assert a[key] == b[key] or key == 'screen_us', key


def test_tree_has_a_few_hundred_leaves():
    ids, live, _, _, _ = directions()
    assert 200 <= len(live) <= 2000 and len(live) <= len(ids)


def test_without_screening_the_new_entry_is_the_old_one_bit_for_bit():
    bb = tree()
    ids, live, pis, pi0, _ = directions()
    old, new, kept = bb._native.support_open(ids), bb._native.support_open(ids), bb._native.support_open(ids, duals=True)
    for pi in pis:
        a = old.eval(pi, pi0, tol=1e-6, max_points=16, want_margins=True)
        for ses in (new, kept):   # (screen_tol < 0 asks for nothing: with and without the flag)
            b = ses.eval(pi, pi0, tol=1e-6, max_points=16, want_margins=True, screen_tol=-1.0)
            assert b['screened'] == 0 and b['lp_solved'] == len(live) and b['retried'] == 0
            assert b['min_screened_margin'] == np.inf
            same(a, {k: v for k, v in b.items() if k not in _ffi.CGLP_EXTRA_KEYS})
    sa, sb = old.stats(), new.stats()
    assert all(sa[k] == sb[k] for k in ('leaves', 'dropped', 'evaluations', 'leaf_lps', 'iterations', 'pivots', 'device_bytes'))
    assert kept.stats()['device_bytes'] > sa['device_bytes']
    with pytest.raises(_ffi.MipxError, match='MIPX_SUPPORT_KEEP_DUALS'):
        new.eval(pis[0], pi0, screen_tol=0.0)
    with pytest.raises(_ffi.MipxError, match='MIPX_SUPPORT_KEEP_DUALS'):
        new.eval(pis[0], pi0, retry_cold=True)
    for ses in (old, new, kept):
        ses.close()


def screening_run():
    bb = tree()
    ids, live, pis, pi0, _ = directions()
    ses = bb._native.support_open(ids, duals=True)
    out = []
    for pi in pis:
        scale = scale_of(pi, pi0)
        out.append(ses.eval(pi, pi0, tol=1e-7 * scale, max_points=16, want_margins=True, screen_tol=0.5e-7 * scale))
    st = ses.stats()
    ses.close()
    return out, st


def test_screening_session_against_highs():
    ids, live, pis, pi0, H = directions()
    out, st = screening_run()
    T = len(live)
    assert st['leaf_lps'] == sum(r['lp_solved'] for r in out) + (len(ids) if len(ids) > T else 0)
    for k, (pi, res) in enumerate(zip(pis, out)):
        scale = scale_of(pi, pi0)
        screen_tol = 0.5e-7 * scale
        print('direction', k, 'screened', res['screened'], 'solved', res['lp_solved'], 'smallest screened margin',
              res['min_screened_margin'], 'not optimal', res['not_optimal'], 'screen us', res['screen_us'])
        assert res['screened'] + res['lp_solved'] == T == res['leaves'] and res['not_optimal'] == 0
        assert (res['screened'] == 0) == (k == 0)     # the first evaluation records the duals, the later ones use them
        assert 0 < res['lp_solved']
        true = H[k] - pi0
        margins = res['margins']
        # every margin is a lower bound on the leaf's own, screened or solved
        assert np.all(margins <= true + 1e-9 * scale)
        # a solved leaf's h_t agrees with HiGHS; a leaf that does not agree was screened, so it lies at or above
        # -screen_tol, and there are no more of those than the evaluation screened
        atol = 1e-9 * max(1.0, float(np.abs(H[k]).max()))
        off = np.abs(margins - true) > atol
        print('   leaves off HiGHS', int(off.sum()), 'largest distance of the others', float(np.abs(margins - true)[~off].max()))
        assert np.all(margins[off] >= -screen_tol) and off.sum() <= res['screened']
        assert np.all(~off[margins < -screen_tol])
        if res['screened']:
            assert res['min_screened_margin'] >= -screen_tol and res['min_screened_margin'] in margins
        # the head and the rows stay what they are: the smallest (margin, node id) over screened and solved alike
        order = np.lexsort((live, margins))[:16]
        assert np.array_equal(res['ids'], live[order]) and np.array_equal(bits(res['h'] - pi0), bits(margins[order]))
        assert res['min_margin'] == margins.min() and res['below'] == int((margins < -1e-7 * scale).sum())


def test_two_screening_sessions_agree_bit_for_bit():
    a, sa = screening_run()
    b, sb = screening_run()
    for ra, rb in zip(a, b):
        same(ra, rb)
    assert {k: v for k, v in sa.items() if not k.endswith('_ms')} == {k: v for k, v in sb.items() if not k.endswith('_ms')}


def test_retry_cold_where_no_leaf_fails_changes_nothing():
    bb = tree()
    ids, live, pis, pi0, _ = directions()
    plain, retry = bb._native.support_open(ids), bb._native.support_open(ids, duals=True)
    for pi in pis:
        a = plain.eval(pi, pi0, tol=1e-6, max_points=16, want_margins=True)
        b = retry.eval(pi, pi0, tol=1e-6, max_points=16, want_margins=True, retry_cold=True)
        assert a['not_optimal'] == 0 and b['retried'] == 0 and b['retried_optimal'] == 0 and b['screened'] == 0
        same(a, {k: v for k, v in b.items() if k not in _ffi.CGLP_EXTRA_KEYS})
    # ... and beside the screen
    both = bb._native.support_open(ids, duals=True)
    ref_run, _ = screening_run()
    for pi, want in zip(pis, ref_run):
        scale = scale_of(pi, pi0)
        got = both.eval(pi, pi0, tol=1e-7 * scale, max_points=16, want_margins=True, screen_tol=0.5e-7 * scale, retry_cold=True)
        assert got['retried'] == 0
        same(want, got)
    for ses in (plain, retry, both):
        ses.close()


# ---- the separator -----------------------------------------------------------------------------------------------
def test_screened_in_out_optimum_equals_the_extended_formulations():
    """The 101-leaf case of test_optimum_equals_the_extended_formulations (40 x 20, seed 3, frontier_batch=1,
    node_limit=100), with screen=True and stabilisation=0.5."""
    A, b, _, _, _, _ = random_dense_milp_arrays(N, M, seed=SEED)
    bb = BranchAndBound(generator_model(N, M, SEED), BaseNode, gomory_cuts=False, frontier_batch=1, tree_record=True,
                        node_limit=100)
    bb.solve()
    tol = 1e-7
    default = DisjunctiveSeparator(bb, 0, tol=tol)
    default.solve()
    default.close()
    sep = DisjunctiveSeparator(bb, 0, tol=tol, screen=True, stabilisation=0.5)
    assert 50 <= len(sep.leaf_ids) <= 200
    pi, pi0 = sep.solve()
    print('default', default.stats)
    print('screen, in-out', sep.stats)
    assert pi is not None and sep.stats['converged'] and default.stats['converged']
    x_star = np.asarray(bb.root_node.solution, np.float64)
    L, U = bb._native.node_bounds(sep.leaf_ids)
    want, live = highs_optimum([(A, b, L[k], U[k]) for k in range(len(sep.leaf_ids))], x_star)
    got = float(np.asarray(pi) @ x_star) - pi0
    allowed = (tol + HIGHS_TOL) * scale_of(pi, pi0)
    print('separator', got, 'HiGHS', want, 'difference', got - want, 'allowed', allowed)
    assert live == sep.stats['leaves']
    assert abs(got - want) <= allowed
    worst = np.inf
    for k in range(len(sep.leaf_ids)):   # valid on every leaf, by HiGHS
        status, h = highs.support(np.asarray(pi), A, b, L[k], U[k])
        if status == 0:
            worst = min(worst, h - pi0)
    print('worst margin by HiGHS', worst)
    assert worst >= -1e-7 * scale_of(pi, pi0)
    assert sep.stats['screened'] > 0
    assert sep.stats['leaf_lps'] < default.stats['leaf_lps']
    assert sep.stats['screened'] + sep.stats['leaf_lps'] >= sep.stats['rounds'] * sep.stats['leaves']
    sep.close()


def test_defaults_are_todays_numbers():
    bb = tree()
    out = []
    for kw in (dict(), dict(screen=False, stabilisation=None, retry_cold=False)):
        sep = DisjunctiveSeparator(bb, 0, **kw)
        pi, pi0 = sep.solve()
        assert 'screened' not in sep.stats and not sep._session.duals
        out.append((bits(np.asarray(pi)).copy(), float(pi0), dict(sep.stats)))
        sep.close()
    assert np.array_equal(out[0][0], out[1][0]) and out[0][1:] == out[1][1:]
