"""The clique cuts on the GPU (include/mipx_clique.h): both kernels against the NumPy restatement
(tests/support/clique_reference.py).  The graph: every word of the adjacency and every row status exact, into buffers
filled with a sentinel, at every width where the words or the loops change (one column; one word of literals and one
literal past it; two words; one workgroup of columns and past it; four columns per thread), on one dense and two
sparse rows, on 130 rows and on 1024, with skipped rows, rows of one item and of none, and a pair exactly at the
margin.  The separation on synthetic adjacencies (empty, complete, random at two densities, with junk where the
entry promises to ignore it): status and size exact, pi, pi0 and the efficacy bit for bit.  And the argument checks
of the two entries."""
import functools

import numpy as np
import pytest

from simple_mip_solver_amd import _ffi
from simple_mip_solver_amd.generators import conflict_packing_milp_arrays
from tests.support import clique_reference as ref

pytestmark = pytest.mark.gpu
INF = float('inf')
COLUMNS = [1, 2, 16, 17, 32, 33, 128, 129, 512, 1023, 1024]
SENTINEL = 0xA5A5A5A5


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def box(n):
    """The box of n columns: binaries, but from 8 columns on every eighth column a general integer in [0, 4] and the one
    behind it continuous in [0, 2.5]; column 3 a binary on {2, 3}, column 5 fixed at 1 (from 6 columns on)."""
    l, u = np.zeros(n), np.ones(n)
    ints = np.ones(n, bool)
    if n >= 8:
        u[0::8], u[1::8] = 4.0, 2.5
        ints[1::8] = False
    if n >= 6:
        l[3], u[3] = 2.0, 3.0
        l[5] = 1.0
    return l, u, tuple(np.flatnonzero(ints).tolist())


@functools.lru_cache(maxsize=None)
def instance(n, m, kind):
    """m knapsack rows over n columns in box(n).  'int': integer weights 1..30; 'real': weights that are no integers.  A
    quarter of the weights is negative; rows 0, 3, 6, ... are dense, the others keep about 12 nonzeros (with m = 1024
    every row is sparse); the general-integer and continuous columns have small coefficients.  The capacity W is 0.7 to
    1.9 times the row's heaviest weight, so that the heavy pairs conflict and the light ones do not.  Row 1 (where
    there is one) asks for more than the box holds (W < 0: skipped)."""
    rng = np.random.default_rng(7000 * n + 10 * m + (kind == 'real'))
    l, u, ints = box(n)
    G = rng.integers(1, 31, (m, n)).astype(np.float64)
    if kind == 'real':
        G = G + rng.random((m, n)) * 0.75
    G *= np.where(rng.random((m, n)) < 0.25, -1.0, 1.0)
    keep = rng.random((m, n)) < min(1.0, 12.0 / n)
    if m < 1024:
        keep[0::3] = True
    G *= keep
    if n >= 8:
        G[:, 0::8] *= 0.125
        G[:, 1::8] *= 0.125
    K = (np.where(G > 0, G * l, G * u)).sum(1)   # (what the row takes at the bounds that help it)
    W = rng.uniform(0.7, 1.9, m) * np.abs(G).max(1)
    if kind == 'int':
        W = np.floor(W)
    d = K + W
    if m >= 2:
        d[1] = K[1] - 1.0
    A, b = 0.0 - G, 0.0 - d
    for a in (A, b, l, u):
        a.setflags(write=False)
    return A, b, l, u, ints


def graph_call(p, l, u, ints):
    """mipx_clique_graph into buffers filled with a sentinel (the bits at 2n and above included)."""
    n, m = p.n, p.m
    adj = np.full((2 * n, ref.words(n)), SENTINEL, np.uint32)
    status = np.full(m, -7, np.int32)
    ii = np.ascontiguousarray(ints, np.int32)
    rc = _ffi.lib().mipx_clique_graph(p._h, _ffi._ptr(np.ascontiguousarray(l)), _ffi._ptr(np.ascontiguousarray(u)),
                                      _ffi._ptr(ii), len(ii), _ffi._ptr(adj), _ffi._ptr(status))
    p.ctx.check(rc, 'mipx_clique_graph')
    assert p.ctx.last_kernel_ms() > 0
    return adj, status


def compare_graph(ctx, n, m, kind):
    A, b, l, u, ints = instance(n, m, kind)
    p = _ffi.Problem(ctx, A, b, np.zeros(n))
    adj, status = graph_call(p, l, u, ints)
    p.close()
    exp, exp_status = ref.graph(A, b, l, u, ints)
    edges = int(exp.sum()) // 2
    print((n, m, kind), 'edges', edges, 'rows skipped', int((exp_status == 4).sum()))
    assert np.array_equal(status, exp_status)
    assert np.array_equal(adj, ref.pack(exp))   # (every word: the bits at 2n and above are 0)
    live = ref.live_literals(l, u, ints)
    assert not exp[~live].any() and np.array_equal(exp, exp.T) and not exp.diagonal().any()
    assert not exp[np.arange(2 * n), np.arange(2 * n) ^ 1].any()
    return edges, exp_status


@pytest.mark.parametrize('kind', ['int', 'real'])
@pytest.mark.parametrize('n', COLUMNS)
def test_the_graph_of_three_rows_equals_the_restatement(n, kind, gpu_ctx):
    edges, status = compare_graph(gpu_ctx, n, 3, kind)
    assert status[1] == 4 and status[0] == status[2] == 0
    assert edges >= 1 or n < 16


@pytest.mark.parametrize('n', [2, 65, 1024])
def test_the_graph_of_130_rows_equals_the_restatement(n, gpu_ctx):
    edges, _ = compare_graph(gpu_ctx, n, 130, 'real')
    assert edges >= 1
    compare_graph(gpu_ctx, n, 130, 'int')


def test_the_graph_of_1024_sparse_rows_equals_the_restatement(gpu_ctx):
    edges, _ = compare_graph(gpu_ctx, 1024, 1024, 'int')
    assert edges >= 1000


def margin_capacities():
    """Two neighbouring doubles W around 2 / (1 + 1e-9): with the first (1 + 1) - W > 1e-9 * max(1, W) holds, with the
    second it does not."""
    W = 2.0 / (1.0 + 1e-9)
    holds = lambda W: (1.0 + 1.0) - W > 1e-9 * max(1.0, abs(W))
    while holds(W):
        W = np.nextafter(W, INF)
    while not holds(W):
        W = np.nextafter(W, -INF)
    assert holds(W) and not holds(np.nextafter(W, INF))
    return float(W), float(np.nextafter(W, INF))


def test_the_content_cases_of_the_graph(gpu_ctx):
    """Rows that end skipped (an infinite bound on a column that is no binary; W < 0), a row with one item, a row with
    none, an empty row, a pair exactly at the margin on both sides, a complemented pair, and a repeated edge."""
    n = 10
    l, u = np.zeros(n), np.ones(n)
    u[8], u[9] = INF, 6.0   # column 8 a continuous column without an upper bound, column 9 a general integer
    ints = [0, 1, 2, 3, 4, 5, 6, 7, 9]
    W_in, W_out = margin_capacities()
    rows = [
        ([3.0, 3.0, 0, 0, 0, 0, 0, 0, -1.0, 0], 4.0),    # 0: needs the infinite bound of column 8: skipped
        ([3.0, 3.0, 0, 0, 0, 0, 0, 0, 1.0, 0], 4.0),     # 1: column 8 relaxed out at l: the edge (0, 2)
        ([3.0, 3.0, 0, 0, 0, 0, 0, 0, 0, 0], -1.0),      # 2: W < 0: skipped
        ([0, 0, 5.0, 0, 0, 0, 0, 0, 0, 2.0], 1.0),       # 3: one item (the general integer is relaxed out): no edge
        ([0, 0, 0, 0, 0, 0, 0, 0, 0, 2.0], 1.0),         # 4: no item
        ([0.0] * n, 0.0),                                  # 5: an empty row
        ([0, 0, 0, 1.0, 1.0, 0, 0, 0, 0, 0], W_in),      # 6: exactly past the margin: the edge (6, 8)
        ([0, 0, 0, 0, 1.0, 1.0, 0, 0, 0, 0], W_out),     # 7: exactly at the margin: no edge
        ([0, 0, 0, 0, 0, 0, -4.0, -4.0, 0, 0], -3.0),    # 8: both complemented, W = 5: the edge (13, 15)
        ([3.0, 3.0, 0, 0, 0, 0, 0, 0, 0, 0], 5.0),       # 9: the edge (0, 2) once more
        ([2.0, 0, 0, 0, 0, 0, 0, -2.0, 0, 0], 0.0),      # 10: W = 2: the edge (0, 15)
    ]
    G = np.array([r for r, _ in rows], np.float64)
    d = np.array([v for _, v in rows])
    A, b = 0.0 - G, 0.0 - d
    p = _ffi.Problem(gpu_ctx, A, b, np.zeros(n))
    adj, status = graph_call(p, l, u, ints)
    exp, exp_status = ref.graph(A, b, l, u, ints)
    assert status.tolist() == exp_status.tolist() == [4, 0, 4, 0, 0, 0, 0, 0, 0, 0, 0]
    assert np.array_equal(adj, ref.pack(exp))
    assert {(int(k), int(h)) for k, h in np.argwhere(exp) if k < h} == {(0, 2), (6, 8), (13, 15), (0, 15)}
    # the wrapper: the same words, the same statuses, NULL for the row status
    got = p.conflict_graph(l, u, ints)
    assert np.array_equal(got['adj'], adj) and np.array_equal(got['row_status'], status) and got['kernel_us'] > 0
    again = np.full_like(adj, SENTINEL)
    rc = _ffi.lib().mipx_clique_graph(p._h, _ffi._ptr(l), _ffi._ptr(u), _ffi._ptr(np.array(ints, np.int32)), len(ints),
                                      _ffi._ptr(again), None)
    assert rc == 0 and np.array_equal(again, adj)
    # a box that fixes column 1: its literals are not live any more, row 1 and row 9 lose their edge
    u2 = u.copy()
    u2[1] = 0.0
    adj2, _ = graph_call(p, l, u2, ints)
    exp2, _ = ref.graph(A, b, l, u2, ints)
    assert np.array_equal(adj2, ref.pack(exp2)) and not exp2[2].any() and exp2.sum() == exp.sum() - 2
    p.close()


# ---- the separation on synthetic adjacencies --------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def synthetic(n, graph):
    """An adjacency over box(n), clean (boolean, among the live literals) and as the words handed to the entry, with
    junk where the entry ignores it: bits at 2n and above, rows and bits of literals that are not live, neither
    symmetric.  65 points with many exact 0s, 0.5s and 1s (in units of the box)."""
    rng = np.random.default_rng(31 * n + len(graph))
    l, u, ints = box(n)
    live = ref.live_literals(l, u, ints)
    k2 = 2 * n
    if graph == 'empty':
        B = np.zeros((k2, k2), bool)
    elif graph == 'complete':
        B = np.zeros((k2, k2), bool)
        B[0::2, 0::2] = True
    else:
        B = np.triu(rng.random((k2, k2)) < float(graph), 1)
        B = B | B.T
    B[np.arange(k2), np.arange(k2)] = False
    B[np.arange(k2), np.arange(k2) ^ 1] = False
    B &= live[:, None] & live[None, :]
    junk = rng.random((k2, 32 * ref.words(n))) < 0.3
    junk[:, :k2] &= ~(live[:, None] & live[None, :])
    words = ref.pack(B) | pack_wide(junk)
    X = rng.random((65, n))
    where = rng.random((65, n))
    X = l + np.where(where < 0.25, 0.0, np.where(where < 0.5, 0.5, np.where(where < 0.65, 1.0, X))) * np.where(np.isfinite(u), u - l, 1.0)
    for a in (B, words, X):
        a.setflags(write=False)
    return l, u, ints, B, words, X


def pack_wide(M):
    """A boolean (rows, 32 Wd) matrix as (rows, Wd) words."""
    M = np.asarray(M, np.uint64)
    return (M.reshape(M.shape[0], -1, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)


def separate_call(p, X, l, u, ints, words, seeds, min_efficacy):
    """mipx_clique_separate_batch into buffers filled with sentinels."""
    n = p.n
    X = np.ascontiguousarray(X, np.float64).reshape(-1, n)
    B = X.shape[0]
    sd = None if seeds is None else np.ascontiguousarray(seeds, np.int32)
    R = 2 * n if sd is None else len(sd)
    ii = np.ascontiguousarray(ints, np.int32)
    out = dict(pi=np.full((B, R, n), -77.5), pi0=np.full((B, R), -77.5), efficacy=np.full((B, R), -77.5),
               size=np.full((B, R), -7, np.int32), status=np.full((B, R), -7, np.int32))
    rc = _ffi.lib().mipx_clique_separate_batch(
        p._h, B, _ffi._ptr(X), _ffi._ptr(np.ascontiguousarray(l)), _ffi._ptr(np.ascontiguousarray(u)), _ffi._ptr(ii), len(ii),
        _ffi._ptr(np.ascontiguousarray(words)), _ffi._ptr(sd), 0 if sd is None else R, float(min_efficacy),
        _ffi._ptr(out['pi']), _ffi._ptr(out['pi0']), _ffi._ptr(out['efficacy']), _ffi._ptr(out['size']), _ffi._ptr(out['status']))
    p.ctx.check(rc, 'mipx_clique_separate_batch')
    assert p.ctx.last_kernel_ms() > 0
    return out


def compare_separation(ctx, n, graph, batch, seeds, check_points, min_efficacy=1e-6, max_seeds=12):
    l, u, ints, B, words, X = synthetic(n, graph)
    p = _ffi.Problem(ctx, np.ones((1, n)), np.zeros(1), np.zeros(n))   # (the rows take no part in the separation)
    got = separate_call(p, X[:batch], l, u, ints, words, seeds, min_efficacy)
    p.close()
    seed_ids = list(range(2 * n)) if seeds is None else list(seeds)
    R = len(seed_ids)
    assert np.all(np.isin(got['status'], (0, 1, 2, 4)))
    check_points = [q for q in check_points if q < batch]
    sel = sorted(set(np.linspace(0, R - 1, min(R, max_seeds)).astype(int).tolist()))
    exp = ref.separate(X[check_points], l, u, ints, B, [seed_ids[k] for k in sel], min_efficacy)
    seen = set()
    for k, q in enumerate(check_points):
        for j, r in enumerate(sel):
            where = (n, graph, batch, q, seed_ids[r])
            print(where, 'status', got['status'][q, r], exp['status'][k, j], 'size', got['size'][q, r], exp['size'][k, j],
                  'efficacy', got['efficacy'][q, r])
            assert got['status'][q, r] == exp['status'][k, j], where
            assert got['size'][q, r] == exp['size'][k, j], where
            assert np.array_equal(bits(got['pi'][q, r]), bits(exp['pi'][k, j])), where
            assert bits(got['pi0'][q, r]) == bits(exp['pi0'][k, j]), where
            assert bits(got['efficacy'][q, r]) == bits(exp['efficacy'][k, j]), where
            seen.add(int(exp['status'][k, j]))
    # seeds that were not compared: what must hold of any output
    none = np.isin(got['status'], (ref.NO_CLIQUE, ref.SKIPPED))
    assert not got['pi'][none].any() and not got['pi0'][none].any() and not got['size'][none].any()
    assert not got['efficacy'][none].any()
    assert np.all(got['size'][~none] >= 2) and np.all(np.isin(got['pi'], (-1.0, 0.0, 1.0)))
    assert np.array_equal(np.abs(got['pi']).sum(axis=2)[~none], got['size'][~none])
    live = ref.live_literals(l, u, ints)
    assert np.all((got['status'] == ref.SKIPPED) == ~live[seed_ids][None, :])
    assert not got['pi'][:, :, ~live[0::2]].any()
    return got, seen


@pytest.mark.parametrize('graph', ['empty', 'complete', '0.5', '0.05'])
@pytest.mark.parametrize('n', COLUMNS)
def test_the_separation_equals_the_restatement(n, graph, gpu_ctx):
    """Every literal a seed (seeds NULL), batch 3; at the widest the complete graph takes a round per binary."""
    got, seen = compare_separation(gpu_ctx, n, graph, 3, None, [0, 2], max_seeds=12 if n <= 129 else 6)
    if graph == 'empty':
        assert not np.isin(got['status'], (ref.CUT, ref.SHALLOW)).any()
    if graph == 'complete' and n >= 16:
        l, u, ints, B, words, X = synthetic(n, graph)
        binaries = int(ref.binary_columns(l, u, ints).sum())
        started = np.isin(got['status'][:, 0::2], (ref.CUT, ref.SHALLOW))
        assert started.any() and np.all(got['size'][:, 0::2][started] == binaries)
        assert np.all(got['status'][:, 1::2][:, ref.live_literals(l, u, ints)[1::2]] == ref.NO_CLIQUE)


@pytest.mark.parametrize('n', [64, 1024])
def test_a_clique_of_every_column(n, gpu_ctx):
    """n binaries and the complete graph on their plain literals: n - 1 rounds, the longest the loop runs; ties at 0.5
    and at 0 everywhere."""
    l, u, ints = np.zeros(n), np.ones(n), list(range(n))
    B = np.zeros((2 * n, 2 * n), bool)
    B[0::2, 0::2] = True
    np.fill_diagonal(B, False)
    X = np.full((2, n), 0.5)
    X[1, 1::3] = 0.0
    X[1, 2::7] = 1.0
    seeds = [2 * n - 2, 0, 2, 1, 2 * (n // 2)]
    p = _ffi.Problem(gpu_ctx, np.ones((1, n)), np.zeros(1), np.zeros(n))
    got = separate_call(p, X, l, u, ints, ref.pack(B), seeds, -INF)
    p.close()
    exp = ref.separate(X, l, u, ints, B, seeds, -INF)
    assert np.array_equal(got['status'], exp['status']) and np.array_equal(got['size'], exp['size'])
    for key in ('pi', 'pi0', 'efficacy'):
        assert np.array_equal(bits(got[key]), bits(exp[key])), key
    assert got['size'][0].tolist() == [n, n, n, 0, n] and got['status'][0].tolist() == [0, 0, 0, 1, 0]
    assert np.all(got['pi'][0, 0] == -1.0) and got['pi0'][0, 0] == -1.0


@pytest.mark.parametrize('n', [2, 17, 129, 1024])
def test_a_subset_of_seeds_in_its_own_order_and_a_batch_of_65(n, gpu_ctx):
    subset = [s for s in (2 * n - 1, 0, n, 7, 2 * n - 2, 12, 3) if s < 2 * n]
    subset = list(dict.fromkeys(subset))
    for graph in ('0.5', '0.05'):
        got, _ = compare_separation(gpu_ctx, n, graph, 65, subset, [0, 31, 64])
        l, u, ints, B, words, X = synthetic(n, graph)
        p = _ffi.Problem(gpu_ctx, np.ones((1, n)), np.zeros(1), np.zeros(n))
        full = separate_call(p, X[:2], l, u, ints, words, None, 1e-6)
        one = separate_call(p, X[1], l, u, ints, words, subset, 1e-6)   # (batch 1)
        p.close()
        for key in ('pi', 'pi0', 'efficacy', 'size', 'status'):
            assert np.array_equal(got[key][:2], full[key][:, subset]), key
            assert np.array_equal(one[key][0], got[key][1]), key


@pytest.mark.parametrize('n', [16, 33, 512])
def test_the_efficacy_threshold(n, gpu_ctx):
    """-inf keeps every clique as a cut; a threshold inside the range of the efficacies makes some shallow, with the
    same pi, pi0, efficacy and size."""
    all_cuts, seen = compare_separation(gpu_ctx, n, '0.5', 3, None, [0, 1], min_efficacy=-INF)
    assert not (all_cuts['status'] == ref.SHALLOW).any() and (all_cuts['status'] == ref.CUT).any()
    eff = all_cuts['efficacy'][all_cuts['status'] == ref.CUT]
    middle = float(np.median(eff))
    some, seen = compare_separation(gpu_ctx, n, '0.5', 3, None, [0, 1], min_efficacy=middle)
    assert {ref.CUT, ref.SHALLOW} <= set(some['status'].ravel().tolist())
    assert np.array_equal(some['status'] == ref.SHALLOW, (all_cuts['status'] == ref.CUT) & ~(all_cuts['efficacy'] > middle))
    for key in ('pi', 'pi0', 'efficacy', 'size'):
        assert np.array_equal(some[key], all_cuts[key]), key


def test_the_cuts_at_one_half_on_the_conflict_family(gpu_ctx):
    """Graph and separation together at x = 0.5 on 24 x 74: 15 / 16 / 17 distinct cuts of sizes 3 to 7 / 3 to 5 /
    3 to 5 (the restatement's figures), every output that of the restatement."""
    for seed, (count, lo, hi) in enumerate([(15, 3, 7), (16, 3, 5), (17, 3, 5)]):
        A, b, c, l, u, ints = conflict_packing_milp_arrays(24, 70, 4, 8, seed=seed)
        p = _ffi.Problem(gpu_ctx, A, b, c)
        g = p.conflict_graph(l, u, ints)
        exp_adj, exp_status = ref.graph(A, b, l, u, ints)
        assert np.array_equal(g['adj'], ref.pack(exp_adj)) and np.array_equal(g['row_status'], exp_status)
        got = p.clique_separate_batch(np.full((1, 24), 0.5), l, u, ints, g['adj'])
        p.close()
        exp = ref.separate(np.full((1, 24), 0.5), l, u, ints, exp_adj)
        assert np.array_equal(got['status'], exp['status']) and np.array_equal(got['size'], exp['size'])
        for key in ('pi', 'pi0', 'efficacy'):
            assert np.array_equal(bits(got[key]), bits(exp[key])), key
        places = ref.distinct_cuts(got)
        sizes = got['size'][0, places]
        assert (len(places), sizes.min(), sizes.max()) == (count, lo, hi) and got['kernel_us'] > 0


def test_the_refused_arguments(gpu_ctx):
    A, b, c, l, u, ints = conflict_packing_milp_arrays(16, 36, 3, 6, seed=0)
    p = _ffi.Problem(gpu_ctx, A, b, c)
    adj = p.conflict_graph(l, u, ints)['adj']
    X = np.full((3, 16), 0.5)
    lbad, ubad, uninf = l.copy(), u.copy(), u.copy()
    lbad[0], ubad[3], uninf[1] = -INF, np.nan, -INF
    for bad in (dict(l=lbad), dict(u=ubad), dict(u=uninf), dict(integer_indices=[0, 0, 1]), dict(integer_indices=[16]),
                dict(integer_indices=[-1])):
        kw = dict(l=l, u=u, integer_indices=list(ints))
        kw.update(bad)
        with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL'):
            p.conflict_graph(**kw)
    ii = np.array(ints, np.int32)
    assert _ffi.lib().mipx_clique_graph(p._h, _ffi._ptr(l), _ffi._ptr(u), _ffi._ptr(ii), 16, None, None) == -1
    assert _ffi.lib().mipx_clique_graph(p._h, None, _ffi._ptr(u), _ffi._ptr(ii), 16, _ffi._ptr(adj.copy()), None) == -1
    # the three faults of an adjacency: not symmetric, a diagonal bit, the two literals of a column joined
    one_way, diagonal, partner = adj.copy(), adj.copy(), adj.copy()
    k, h = next((k, h) for k in range(32) for h in range(32) if k != h and k != h ^ 1 and not adj[k, 0] >> h & 1)
    one_way[k, 0] |= np.uint32(1 << h)
    diagonal[4, 0] |= np.uint32(1 << 4)
    partner[6, 0] |= np.uint32(1 << 7)
    partner[7, 0] |= np.uint32(1 << 6)
    Xbad = X.copy()
    Xbad[1, 4] = np.nan
    for bad in (dict(adj=one_way), dict(adj=diagonal), dict(adj=partner), dict(X=Xbad), dict(l=lbad), dict(u=ubad),
                dict(u=uninf), dict(integer_indices=[0, 0, 1]), dict(integer_indices=[16]), dict(integer_indices=[-1]),
                dict(seeds=[0, 0]), dict(seeds=[32]), dict(seeds=[-1]), dict(seeds=[]), dict(min_efficacy=float('nan'))):
        kw = dict(X=X, l=l, u=u, integer_indices=list(ints), adj=adj)
        kw.update(bad)
        with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL'):
            p.clique_separate_batch(**kw)
    # the same faults on literals that are not live are junk, and ignored
    fewer = [j for j in ints if j not in (2, 3)]
    for words in (diagonal, partner):
        got = p.clique_separate_batch(X, l, u, fewer, words)
        exp = ref.separate(X, l, u, fewer, ref.unpack(adj, 16))
        assert np.array_equal(got['status'], exp['status']) and np.array_equal(bits(got['pi']), bits(exp['pi']))
    ok = p.clique_separate_batch(X, l, u, ints, adj, seeds=[31, 0])
    assert ok['pi'].shape == (3, 2, 16) and ok['size'].shape == (3, 2)
    empty = p.clique_separate_batch(np.zeros((0, 16)), l, u, ints, adj)
    assert empty['pi'].shape == (0, 32, 16) and empty['kernel_us'] == 0.0
    p.close()
