"""The kernels behind a support evaluation (csrc/cglp_kernels.hip.h, csrc/cglp_screen_kernels.hip.h) on synthetic
leaves, through the entries of include/mipx_supportkernels.h (the launches the session uses: the enqueue_support_*
functions) and, for support_screen, through mipx_support_screen_batch, against the NumPy restatement in
tests/support/support_kernels_reference.py: the selection at 1 .. 258 segments, 1 .. 1024 rows asked for and widths
1 .. 1024, with ties, missing leaves, empty segments and objectives that are not finite; the packing in both modes at
every density; the gather, the scatter with LPs that FAIL, the mark; the screen at 1023 and 1024 rows and columns;
and one evaluation chained entry by entry whose retry has leaves that fail once and leaves that fail twice, which no
session can produce.  Every output buffer goes in filled with 0x5a and is compared whole: what the restatement does
not write must still be 0x5a.  Nothing here is a tolerance: every comparison is of bits."""
import numpy as np
import pytest

from tests.support import cglp_screen_reference as screen_ref
from tests.support import support_kernels_reference as ref

pytestmark = pytest.mark.gpu
SEG = ref.SEG


def ffi():
    from simple_mip_solver_amd import _ffi
    return _ffi


def agree(got, want, what):
    for k in want:
        assert ref.same_bits(got[k], want[k]), (what, k)


# ---- select + merge ------------------------------------------------------------------------------------------------------
def run_select(ctx, c):
    got = ref.select_buffers(c)
    ffi().support_select_batch(ctx, c['T'], c['n'], c['P'], c['pi0'], c['tol'], c['ids'], c['status'], c['obj'], c['x'], c['iters'],
                               c['npivots'], got['margin'], got['cand_m'], got['cand_id'], got['cand_t'], got['seg_sum'], got['block'])
    return got


def check_select(ctx, c):
    what = (c['content'], c['T'], c['n'], c['P'])
    print(what, c['kinds'])
    want = ref.select(c, ref.select_buffers(c))
    got = run_select(ctx, c)
    agree(got, want, what)
    nsel = int(want['block'][3])
    assert nsel == min(c['P'], c['kinds']['ok'])
    assert ref.untouched(got['block'][ref.HEAD + nsel * (c['n'] + 2):])   # the rows past nsel are not written
    return want


@pytest.mark.parametrize('P', ref.ROWS_ASKED)
@pytest.mark.parametrize('T', ref.SIZES)
def test_select_at_every_size_and_every_number_of_rows(gpu_ctx, T, P):
    c = ref.select_case('mixed', T, 2, P)
    check_select(gpu_ctx, c)
    if T >= 255:
        k = c['kinds']
        assert k['status_bad'] and k['nan'] and k['pos_inf'] and k['neg_inf'] and k['tie_pairs'] and k['ids_unordered']
        assert k['max_id'] == ref.MAX_ID


@pytest.mark.parametrize('n', ref.WIDTHS)
def test_select_rows_at_every_width(gpu_ctx, n):
    for T, P in ((300, 16), (5, 16), (2049, 3)):
        check_select(gpu_ctx, ref.select_case('mixed', T, n, P))


@pytest.mark.parametrize('content', [c for c in ref.CONTENTS if c != 'mixed'])
@pytest.mark.parametrize('P', (1, 16, 1024))
def test_select_content_cases(gpu_ctx, content, P):
    T = 3 * SEG + 5
    c = ref.select_case(content, T, 2, P)
    want = check_select(gpu_ctx, c)
    k, head = c['kinds'], want['block'][:ref.HEAD]
    if content == 'ties':
        assert k['ties_across_segments'] and k['ties_descending_ids'] and k['neg_zero'] and k['tie_pairs'] > T // 2
    if content == 'empty-segment':
        assert k['empty_segments'] == 1 and ref.same_bits(want['cand_id'][1], np.full(P, ref.NONE, np.int32))
    if content == 'none-ok':
        assert k['ok'] == 0 and k['nan'] and head[3] == 0 and head[0] == ref.INF and head[1] == -1 and head[4] == T
    if content == 'few-ok':
        assert (P == 1 or k['short_segments'] >= 1) and (P <= 3 or (k['short_overall'] and 0 < head[3] < P))
    if content == 'tol-edge':
        assert k['at_tol'] and k['just_below_tol'] and head[2] == k['just_below_tol'] + int((ref.margins(c) <= -0.75).sum())
    if content == 'big-counts':
        assert k['iters_total'] > 2 ** 32 and k['pivots_total'] > 2 ** 32 and head[5] == k['iters_total'] and head[6] == k['pivots_total']


@pytest.mark.parametrize('T, P, content', [(ref.T_65, 16, 'big-counts'), (ref.T_WAVES, 1, 'mixed'), (ref.T_WAVES, 16, 'mixed'), (ref.T_WAVES, 16, 'big-counts'),
                                           (ref.T_TWICE, 2, 'mixed'), (ref.T_TWICE, 16, 'big-counts'), (ref.T_TWICE, 16, 'ties'),
                                           (ref.T_TWICE, 1024, 'mixed')])
def test_select_beyond_one_wave_of_segments(gpu_ctx, T, P, content):
    """From 65 segments on wave 0 of the merge no longer holds every segment's sums (65 and 66 here); from 257 on a thread
    takes two (258 here)."""
    c = ref.select_case(content, T, 1, P)
    want = check_select(gpu_ctx, c)
    assert want['block'][7] == T and want['block'][5] == c['kinds']['iters_total']
    assert np.asarray(c['iters'][64 * SEG:], np.int64).sum() > 0 and (T < ref.T_TWICE or np.asarray(c['iters'][256 * SEG:], np.int64).sum() > 0)


# ---- pack ----------------------------------------------------------------------------------------------------------------
def run_pack(ctx, T, mode, pi0, skip, status, bound):
    got = ref.pack_buffers(T)
    ffi().support_pack_batch(ctx, T, mode, pi0, skip, status, bound, got['seg_count'], got['seg_min'], got['packed'], got['count'],
                             got['min_margin'])
    return got


def check_pack(ctx, c, mode, with_bound):
    T = c['T']
    poison = np.full(T, np.nan)
    skip, status = (c['skip'], None) if mode == 0 else (np.full(T, ref.FILL, np.uint8), c['status'])
    bound = (c['bound'] if with_bound else None) if mode == 0 else poison
    want = ref.pack(T, mode, c['pi0'], skip, status, bound, ref.pack_buffers(T))
    got = run_pack(ctx, T, mode, c['pi0'], skip, status, bound)
    agree(got, want, (T, mode, with_bound))
    count = int(want['count'][0])
    assert count == int(c['take'].sum()) and ref.untouched(got['packed'][count:])
    if mode == 1 or not with_bound:
        assert got['min_margin'][0] == ref.INF and np.all(got['seg_min'] == ref.INF)
    return want


@pytest.mark.parametrize('T', ref.SIZES + (ref.T_65, ref.T_WAVES, ref.T_TWICE))
def test_pack_at_every_size_and_density(gpu_ctx, T):
    seen = {}
    for density in ref.DENSITIES:
        c = ref.pack_case(density, T)
        seen[density] = int(c['take'].sum())
        want = check_pack(gpu_ctx, c, 0, True)
        assert want['min_margin'][0] == (-7.625 - c['pi0'] if c['at'] >= 0 else ref.INF)
        check_pack(gpu_ctx, c, 0, False)
        check_pack(gpu_ctx, c, 1, False)
    print(T, seen)
    assert seen['none'] == 0 and seen['all'] == T and seen['first'] == seen['last'] == 1
    if T >= 3 * SEG:
        c = ref.pack_case('empty-middle-segment', T)
        assert not c['take'][(ref.segments(T) // 2) * SEG:(ref.segments(T) // 2 + 1) * SEG].any() and 0.3 * T < seen['half'] < 0.7 * T


@pytest.mark.parametrize('T', (2049, 3 * SEG + 5, ref.T_WAVES, ref.T_TWICE))
@pytest.mark.parametrize('spot', ref.MARGIN_SPOTS)
def test_pack_min_margin_wherever_it_sits(gpu_ctx, T, spot):
    c = ref.pack_case('half' if spot != 'absent' else 'all', T, spot)
    want = check_pack(gpu_ctx, c, 0, True)
    G, at = ref.segments(T), c['at']
    print(T, spot, at, want['min_margin'][0])
    if spot == 'absent':
        assert want['min_margin'][0] == ref.INF and c['take'].all()
    else:
        assert want['min_margin'][0] == -7.625 - c['pi0'] and want['seg_min'][at // SEG] == want['min_margin'][0]
        assert {'last-segment': at // SEG == G - 1, 'first-segment': at < SEG, 'last-item-of-a-thread': at % 8 == 7}[spot]
        # the taken leaves carry far smaller bounds: a minimum over the wrong leaves would show
        assert (c['bound'][c['take']] - c['pi0']).min() < want['min_margin'][0]


# ---- gather, scatter, mark -----------------------------------------------------------------------------------------------
def move_cases():
    return [(n, m, T, count) for n, m in ref.MOVE_SHAPES for T in ref.MOVE_LEAVES for count in ref.move_counts(T)]


@pytest.mark.parametrize('n, m', ref.MOVE_SHAPES)
def test_gather_warm_and_cold(gpu_ctx, n, m):
    for T in ref.MOVE_LEAVES:
        for count in ref.move_counts(T):
            c = ref.move_case(n, m, T, count)
            leaf = c['leaf']
            for v in (leaf['v'], None):
                shapes = (((count, n), np.float64), ((count, n), np.float64), ((count, n + m), np.int8))
                want, got = ([ref.filled(*s) for s in shapes] for _ in range(2))
                ref.gather(count, c['packed'], leaf['l'], leaf['u'], v, *want)
                ffi().support_gather_batch(gpu_ctx, count, T, n, m, c['packed'], leaf['l'], leaf['u'], v, *got)
                for g, w, k in zip(got, want, ('pl', 'pu', 'pv_in')):
                    assert ref.same_bits(g, w), (n, m, T, count, v is None, k)
                assert v is not None or ref.untouched(got[2])        # the cold gather leaves the codes alone
                assert count == 0 or not ref.untouched(got[0])


@pytest.mark.parametrize('add', (0, 1))
@pytest.mark.parametrize('n, m', ref.MOVE_SHAPES)
def test_scatter_with_lps_that_fail(gpu_ctx, n, m, add):
    outcomes = set()
    for T in ref.MOVE_LEAVES:
        for count in ref.move_counts(T):
            c = ref.move_case(n, m, T, count)
            lp, packed = c['lp'], c['packed']
            want, got = ({k: c['leaf'][k].copy() for k in ref.LEAF_KEYS} for _ in range(2))
            ref.scatter(count, packed, add, lp, want)
            ffi().support_scatter_batch(gpu_ctx, count, T, n, m, packed, add, lp['px'], lp['pobj'], lp['py'], lp['pv_out'], lp['pstatus'],
                                        lp['piters'], lp['pnpivots'], *(got[k] for k in ref.LEAF_KEYS))
            agree(got, want, (n, m, T, count, add))
            before = c['leaf']
            rest = np.setdiff1d(np.arange(T), packed)
            for k in ref.LEAF_KEYS:                                  # the leaves that are not packed stay
                assert ref.same_bits(got[k][rest], before[k][rest]), k
            for k in range(count):
                t, failed = packed[k], lp['pstatus'][k] != 0
                outcomes.add((bool(before['has_y'][t]), bool(failed)))
                if failed:                                           # a failed LP keeps the leaf's duals and its has_y
                    assert ref.same_bits(got['y'][t], before['y'][t]) and got['has_y'][t] == before['has_y'][t]
                    assert got['status'][t] == lp['pstatus'][k] and ref.same_bits(got['x'][t], lp['px'][k])
                else:
                    assert got['has_y'][t] == 1
                assert got['iters'][t] == lp['piters'][k] + (before['iters'][t] if add else 0)
    print((n, m, add), sorted(outcomes))
    assert outcomes == {(False, False), (False, True), (True, False), (True, True)}


def test_scatter_into_sentinel_leaves(gpu_ctx):
    """Leaf-side arrays of 0x5a: the rows of the leaves that are not packed, and the duals of a failed leaf, stay 0x5a."""
    c = ref.move_case(257, 255, 300, 150)
    lp, packed, n, m, T = c['lp'], c['packed'], 257, 255, 300
    dtypes = dict(x=((T, n), np.float64), obj=(T, np.float64), y=((T, m), np.float64), v=((T, n + m), np.int8), status=(T, np.int32),
                  iters=(T, np.int32), npivots=(T, np.int32), has_y=(T, np.uint8))
    want, got = ({k: ref.filled(*dtypes[k]) for k in ref.LEAF_KEYS} for _ in range(2))
    ref.scatter(150, packed, 0, lp, want)
    ffi().support_scatter_batch(gpu_ctx, 150, T, n, m, packed, 0, lp['px'], lp['pobj'], lp['py'], lp['pv_out'], lp['pstatus'], lp['piters'],
                                lp['pnpivots'], *(got[k] for k in ref.LEAF_KEYS))
    agree(got, want, 'sentinel')
    rest = np.setdiff1d(np.arange(T), packed)
    failed = packed[lp['pstatus'] != 0]
    assert len(failed) and len(failed) < 150
    for k in ref.LEAF_KEYS:
        assert ref.untouched(got[k][rest]), k
    assert ref.untouched(got['y'][failed]) and ref.untouched(got['has_y'][failed]) and not ref.untouched(got['x'][failed])


@pytest.mark.parametrize('T', (1, 255, 256, 257, 2049))
def test_mark(gpu_ctx, T):
    rng = np.random.default_rng(T)
    status = (rng.integers(0, 4, T) * (rng.random(T) < 0.5)).astype(np.int32)
    status[-1] = 3 if T > 1 else 0
    for before in (0, 1, ref.FILL):
        got, want = np.full(T + 3, before, np.uint8), np.full(T + 3, before, np.uint8)
        ref.mark(T, status, want)
        ffi().support_mark_batch(gpu_ctx, T, status, got)
        assert ref.same_bits(got, want) and np.all(got[T:] == before)
    assert T == 1 or (0 < (status != 0).sum() < T)                   # a verdict that is not optimal clears the flag


# ---- the screen at its limits ----------------------------------------------------------------------------------------------
def check_screen(p, A, b, pi, pi0, tol, l, u, y, has_y, what):
    want = screen_ref.screen(A, b, pi, pi0, tol, l, u, y, has_y)
    got = p.support_screen_batch(pi, pi0, tol, l, u, y, has_y)
    for k in ('bound', 'screened', 'packed'):
        assert ref.same_bits(got[k], want[k]), (what, k)
    assert got['count'] == want['count']
    return want


@pytest.mark.parametrize('m, n', [(1023, 1023), (1024, 1024), (1024, 1), (1, 1024)])
def test_screen_at_1024_rows_and_columns(gpu_ctx, m, n):
    T = 5                                                        # the last workgroup holds one leaf
    rng = np.random.default_rng(m * 2048 + n)
    A, b = rng.standard_normal((m, n)), rng.standard_normal(m)
    p = ffi().Problem(gpu_ctx, A, b, np.zeros(n))
    try:
        pi = rng.uniform(-1, 1, n)
        l = rng.uniform(-3, 3, (T, n)).round(2)
        u = l + rng.uniform(0, 4, (T, n)).round(2)
        y = rng.uniform(-0.5, 2.0, (T, m)) * (rng.random((T, m)) < 0.4)
        y[:, -1] = 1.5                                           # the last row counts in every leaf
        has_y = np.array([1, 1, 0, 1, 1], np.uint8)
        L = screen_ref.bound(A, b, pi, l, u, y, has_y)
        assert np.all(np.isfinite(L[has_y != 0]))
        want = check_screen(p, A, b, pi, float(np.median(L[has_y != 0])), 1e-7, l, u, y, has_y, (m, n))
        print((m, n), want['count'], want['screened'].tolist())
        assert 0 < want['count'] < T and want['screened'][4] in (0, 1)
    finally:
        p.close()


def test_screen_and_pack_by_skip_beyond_one_wave_of_segments(gpu_ctx):
    T = ref.T_WAVES
    rng = np.random.default_rng(65)
    A, b = np.array([[1.5]]), np.array([0.25])
    p = ffi().Problem(gpu_ctx, A, b, np.zeros(1))
    try:
        l = rng.uniform(-3, 3, (T, 1)).round(2)
        u = l + rng.uniform(0, 4, (T, 1)).round(2)
        y = rng.uniform(-0.5, 2.0, (T, 1))
        has_y = (rng.random(T) < 0.85).astype(np.uint8)
        pi = np.array([0.75])
        r = pi[0] - A[0, 0] * np.maximum(y[:, 0], 0.0)              # (about the bound: only to place pi0 near its median)
        pi0 = float(np.median((np.maximum(y[:, 0], 0.0) * b[0] + np.minimum(r * l[:, 0], r * u[:, 0]))[has_y != 0]))
        want = check_screen(p, A, b, pi, pi0, 1e-7, l, u, y, has_y, '66 segments')
        print(T, want['count'])
        assert 0.4 * T < want['count'] < 0.7 * T and (want['packed'][:want['count']] >= 64 * SEG).any()
        # the same skip list and bounds through the pack entry: the same positions, and the margin the screen entry drops
        got = run_pack(gpu_ctx, T, 0, pi0, want['screened'], None, want['bound'])
        mine = ref.pack(T, 0, pi0, want['screened'], None, want['bound'], ref.pack_buffers(T))
        agree(got, mine, 'pack of the screen')
        assert ref.same_bits(got['packed'][:want['count']], want['packed'][:want['count']])
        assert got['min_margin'][0] == (want['bound'][want['screened'] != 0] - pi0).min() >= -1e-7
    finally:
        p.close()


# ---- one evaluation, entry by entry ------------------------------------------------------------------------------------------
def drawn_evaluation():
    """T = 2049 + 300 leaves of m = 6 rows and n = 9 columns, and the results of two launches drawn per leaf: about one
    first LP in ten fails, and half of those fail again without a basis."""
    T, m, n, P = 2049 + 300, 6, 9, 16
    rng = np.random.default_rng(2349)
    A, b, pi = rng.standard_normal((m, n)), rng.standard_normal(m), rng.uniform(-1, 1, n)
    l = rng.uniform(-3, 3, (T, n)).round(2)
    u = l + rng.uniform(0, 4, (T, n)).round(2)
    ids = ref._ids(rng, T)
    leaf = dict(x=rng.standard_normal((T, n)), obj=rng.standard_normal(T), y=rng.uniform(-0.5, 2.0, (T, m)) * (rng.random((T, m)) < 0.4),
                v=rng.integers(-1, 3, (T, n + m)).astype(np.int8), status=np.zeros(T, np.int32),
                iters=rng.integers(0, 99, T).astype(np.int32), npivots=rng.integers(0, 9, T).astype(np.int32),
                has_y=(rng.random(T) < 0.85).astype(np.uint8))
    L = screen_ref.bound(A, b, pi, l, u, leaf['y'], leaf['has_y'])
    pi0 = float(np.median(L[leaf['has_y'] != 0]))

    def launch(fail):
        return dict(px=rng.standard_normal((T, n)), pobj=(pi0 + rng.integers(-8, 9, T) * 0.125), py=rng.standard_normal((T, m)),
                    pv_out=rng.integers(-1, 3, (T, n + m)).astype(np.int8), pstatus=np.where(fail, rng.integers(1, 4, T), 0).astype(np.int32),
                    piters=rng.integers(1, 99, T).astype(np.int32), pnpivots=rng.integers(1, 9, T).astype(np.int32))
    fail1 = rng.random(T) < 0.10
    fail2 = fail1 & (rng.random(T) < 0.5)
    return dict(T=T, m=m, n=n, P=P, A=A, b=b, pi=pi, pi0=pi0, tol=0.25, screen_tol=1e-7, ids=ids, l=l, u=u, leaf=leaf,
                lp1=launch(fail1), lp2=launch(fail2))


def test_one_evaluation_entry_by_entry_with_leaves_that_fail(gpu_ctx):
    F = ffi()
    e = drawn_evaluation()
    T, m, n, P, pi0, l, u = e['T'], e['m'], e['n'], e['P'], e['pi0'], e['l'], e['u']
    want_leaf = {k: a.copy() for k, a in e['leaf'].items()}
    want = ref.evaluation(e['A'], e['b'], e['pi'], pi0, e['tol'], e['screen_tol'], P, e['ids'], l, u, want_leaf, e['lp1'], e['lp2'])
    leaf = {k: a.copy() for k, a in e['leaf'].items()}
    p = F.Problem(gpu_ctx, e['A'], e['b'], np.zeros(n))
    try:
        scr = p.support_screen_batch(e['pi'], pi0, e['screen_tol'], l, u, leaf['y'], leaf['has_y'])
    finally:
        p.close()
    for k in ('bound', 'screened', 'packed'):
        assert ref.same_bits(scr[k], want['screen'][k]), k
    ref.screen_record(leaf, scr['bound'], scr['screened'])

    def launch(mode, warm, add, lp, want_pack, want_gather, want_after):
        pk = run_pack(gpu_ctx, T, mode, pi0, scr['screened'] if mode == 0 else None, leaf['status'] if mode else None,
                      scr['bound'] if mode == 0 else None)
        agree(pk, want_pack, ('pack', mode))
        count = int(pk['count'][0])
        g = dict(pl=ref.filled((T, n), np.float64), pu=ref.filled((T, n), np.float64), pv_in=ref.filled((T, n + m), np.int8))
        F.support_gather_batch(gpu_ctx, count, T, n, m, pk['packed'][:count], l, u, leaf['v'] if warm else None, g['pl'][:count],
                               g['pu'][:count], g['pv_in'][:count])
        agree(g, want_gather, ('gather', mode))
        rows = ref.lp_rows(lp, pk['packed'], count)
        F.support_scatter_batch(gpu_ctx, count, T, n, m, pk['packed'][:count], add, rows['px'], rows['pobj'], rows['py'], rows['pv_out'],
                                rows['pstatus'], rows['piters'], rows['pnpivots'], *(leaf[k] for k in ref.LEAF_KEYS))
        agree(leaf, want_after, ('scatter', mode))
        return count, rows

    solved, _ = launch(0, True, 0, e['lp1'], want['pack1'], want['gather1'], want['leaf1'])
    assert ref.same_bits(scr['packed'][:solved], want['pack1']['packed'][:solved]) and solved == scr['count']
    retried, rows2 = launch(1, False, 1, e['lp2'], want['pack2'], want['gather2'], want['leaf2'])
    retried_ok = int((rows2['pstatus'] == 0).sum())
    print('leaves', T, 'screened', T - solved, 'solved', solved, 'retried', retried, 'of which optimal', retried_ok)
    assert 0 < solved < T and retried > 0 and 0 < retried_ok < retried        # both outcomes of the retry occur
    assert (retried, retried_ok) == (want['retried'], want['retried_ok'])
    # a leaf that failed twice: its duals and has_y are those from before the evaluation, its counts those of both LPs
    twice = np.flatnonzero(leaf['status'] != 0)
    assert len(twice) == retried - retried_ok
    assert ref.same_bits(leaf['y'][twice], e['leaf']['y'][twice]) and ref.same_bits(leaf['has_y'][twice], e['leaf']['has_y'][twice])
    assert np.array_equal(leaf['iters'][twice], e['lp1']['piters'][twice] + e['lp2']['piters'][twice])
    assert {0, 1} <= set(e['leaf']['has_y'][twice].tolist())
    c = dict(want['select_case'], status=leaf['status'], obj=leaf['obj'], x=leaf['x'], iters=leaf['iters'], npivots=leaf['npivots'])
    got = run_select(gpu_ctx, c)
    agree(got, want['select'], 'select')
    assert got['block'][4] == len(twice) and got['block'][3] == P


# ---- refusals --------------------------------------------------------------------------------------------------------------
def refused(call, word):
    with pytest.raises(ffi().MipxError) as err:
        call()
    assert word in str(err.value), (word, str(err.value))


def test_select_refusals(gpu_ctx):
    c = dict(ref.select_case('mixed', 5, 2, 3))
    keys = ('ids', 'status', 'obj', 'x', 'iters', 'npivots')

    def call(out=None, **over):
        d = dict(c, **over)
        out = out if out is not None else ref.select_buffers(d if d['T'] == 5 and 1 <= d['P'] <= 1024 and d['n'] == 2 else c)
        ffi().support_select_batch(gpu_ctx, d['T'], d['n'], d['P'], d['pi0'], d['tol'], *(d[k] for k in keys), out['margin'], out['cand_m'],
                                   out['cand_id'], out['cand_t'], out['seg_sum'], out['block'])
        return out
    for k in keys:
        refused(lambda: call(**{k: None}), 'null')
    for k in ('margin', 'cand_m', 'cand_id', 'cand_t', 'seg_sum', 'block'):
        refused(lambda: call(out=dict(ref.select_buffers(c), **{k: None})), 'null')
    refused(lambda: call(T=-1), 'T negative')
    refused(lambda: call(T=2 ** 30 + 1), 'T negative or above')
    refused(lambda: call(P=0), 'P outside')
    refused(lambda: call(P=1025), 'P outside')
    refused(lambda: call(n=0), 'n < 1')
    refused(lambda: call(tol=-1e-300), 'tol')
    refused(lambda: call(tol=float('nan')), 'tol')
    refused(lambda: call(pi0=float('nan')), 'pi0')
    for bad in (-1, ref.NONE, 2 ** 31, 2 ** 40):
        ids = c['ids'].copy()
        ids[4] = bad
        out = ref.select_buffers(c)
        refused(lambda: call(out=out, ids=ids), 'id outside')
        assert all(ref.untouched(a) for a in out.values())             # a refused call writes nothing
    agree(call(), ref.select(c, ref.select_buffers(c)), 'a valid call still runs')
    assert all(ref.untouched(a) for a in call(T=0).values())           # T = 0: no launch


def test_pack_refusals(gpu_ctx):
    c = ref.pack_case('half', 300)

    def call(T=300, mode=0, pi0=0.5, skip=c['skip'], status=c['status'], bound=c['bound'], **out):
        bufs = dict(ref.pack_buffers(300), **out)
        ffi().support_pack_batch(gpu_ctx, T, mode, pi0, skip, status, bound, bufs['seg_count'], bufs['seg_min'], bufs['packed'],
                                 bufs['count'], bufs['min_margin'])
        return bufs
    refused(lambda: call(skip=None), 'null')
    refused(lambda: call(mode=1, status=None), 'null')
    for k in ('seg_count', 'seg_min', 'packed', 'count', 'min_margin'):
        refused(lambda: call(**{k: None}), 'null')
    refused(lambda: call(T=-1), 'T negative')
    refused(lambda: call(T=2 ** 30 + 1), 'above 2^30')
    refused(lambda: call(mode=2), 'mode')
    refused(lambda: call(mode=-1), 'mode')
    refused(lambda: call(pi0=float('nan')), 'pi0')
    agree(call(status=None), ref.pack(300, 0, 0.5, c['skip'], None, c['bound'], ref.pack_buffers(300)), 'valid, mode 0')
    agree(call(mode=1, skip=None, bound=None), ref.pack(300, 1, 0.5, None, c['status'], None, ref.pack_buffers(300)), 'valid, mode 1')
    assert all(ref.untouched(a) for a in call(T=0).values())


def test_gather_and_scatter_refusals(gpu_ctx):
    n, m, T, count = 5, 3, 5, 2
    c = ref.move_case(n, m, T, count)
    leaf, lp = c['leaf'], c['lp']

    def gather(count=count, T=T, n=n, m=m, packed=c['packed'], l=leaf['l'], u=leaf['u'], v=leaf['v'], **out):
        bufs = dict(dict(pl=ref.filled((2, 5), np.float64), pu=ref.filled((2, 5), np.float64), pv_in=ref.filled((2, 8), np.int8)), **out)
        ffi().support_gather_batch(gpu_ctx, count, T, n, m, packed, l, u, v, bufs['pl'], bufs['pu'], bufs['pv_in'])
        return bufs

    def scatter(count=count, T=T, n=n, m=m, packed=c['packed'], add=0, **over):
        d = dict(lp, **{k: leaf[k].copy() for k in ref.LEAF_KEYS})
        d.update(over)
        ffi().support_scatter_batch(gpu_ctx, count, T, n, m, packed, add, d['px'], d['pobj'], d['py'], d['pv_out'], d['pstatus'], d['piters'],
                                    d['pnpivots'], *(d[k] for k in ref.LEAF_KEYS))
        return d
    for call in (gather, scatter):
        refused(lambda: call(packed=None), 'null')
        refused(lambda: call(count=-1), 'negative')
        refused(lambda: call(T=-1), 'negative')
        refused(lambda: call(count=2 ** 30 + 1, T=2 ** 30 + 1), 'above 2^30')
        refused(lambda: call(T=2 ** 30 + 1), 'above 2^30')
        refused(lambda: call(count=6), 'count > T')
        refused(lambda: call(n=0), 'n < 1')
        refused(lambda: call(m=-1), 'm < 0')
        refused(lambda: call(packed=np.array([1, 5], np.int32)), 'outside 0 .. T-1')
        refused(lambda: call(packed=np.array([-1, 2], np.int32)), 'outside 0 .. T-1')
    for k in ('l', 'u', 'pl', 'pu', 'pv_in'):
        refused(lambda: gather(**{k: None}), 'null')
    for k in ('px', 'pobj', 'py', 'pv_out', 'pstatus', 'piters', 'pnpivots') + ref.LEAF_KEYS:
        refused(lambda: scatter(**{k: None}), 'null')
    refused(lambda: scatter(packed=np.array([3, 3], np.int32)), 'twice')
    # past the count nothing of packed is read: a wild entry there is no refusal
    wide = np.array([c['packed'][0], c['packed'][1], 99], np.int32)
    want = dict(pl=ref.filled((2, 5), np.float64), pu=ref.filled((2, 5), np.float64), pv_in=ref.filled((2, 8), np.int8))
    ref.gather(2, c['packed'], leaf['l'], leaf['u'], leaf['v'], **want)
    agree(gather(packed=wide), want, 'a valid gather still runs')
    after = {k: leaf[k].copy() for k in ref.LEAF_KEYS}
    ref.scatter(2, c['packed'], 1, lp, after)
    agree({k: v for k, v in scatter(add=1, packed=wide).items() if k in ref.LEAF_KEYS}, after, 'a valid scatter still runs')
    assert all(ref.untouched(a) for a in gather(count=0).values())
    cold = gather(v=None, pv_in=None)
    assert not ref.untouched(cold['pl'])


def test_mark_refusals(gpu_ctx):
    status, has_y = np.array([0, 2, 0], np.int32), np.full(3, ref.FILL, np.uint8)
    refused(lambda: ffi().support_mark_batch(gpu_ctx, 3, None, has_y), 'null')
    refused(lambda: ffi().support_mark_batch(gpu_ctx, 3, status, None), 'null')
    refused(lambda: ffi().support_mark_batch(gpu_ctx, -1, status, has_y), 'T negative')
    refused(lambda: ffi().support_mark_batch(gpu_ctx, 2 ** 30 + 1, status, has_y), 'above 2^30')
    assert ref.untouched(has_y)
    ffi().support_mark_batch(gpu_ctx, 0, status, has_y)
    assert ref.untouched(has_y)
    ffi().support_mark_batch(gpu_ctx, 3, status, has_y)
    assert has_y.tolist() == [1, 0, 1]
