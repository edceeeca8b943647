"""The tree queries (mipx_tree_node_bounds, mipx_tree_node_solve), the support session behind
DisjunctiveSeparator (mipx_tree_support_open / _eval) and the restart (mipx_tree_create_restart) past their first
launch: every one of them works through its nodes in chunks of kTrChunk = 2^14, and the session selects per
segment of kSupSeg = 2048 leaves and then merges the segments' candidates.  The other modules stay inside the
first chunk and the first segment; here every size is derived from those two constants, so that the second trip
of every chunk loop, the merge over several segments, a partial last segment, P at its cap and the
(margin, node id) tie-break all run.

The judges are never the engine: a NumPy walk over the record arrays for the bounds (tests/support/
tree_reference.py), the LP certificates for the re-solve (tests/support/lp_certificate.py), NumPy's lexsort over
the full margins for the selection, HiGHS for h_t and for the dropped leaves (tests/support/cglp_reference.py),
and the project's own pinned property that a node LP does not depend on its place in a batch
(tests/test_lp_kernel_gpu.py) for the chunk-independence checks.

The tree: random_dense_milp_arrays(64, 32, seed=5), pseudo-cost branching, best first, anchors on, a plunge of
depth 2, frontier_batch = 1024, mip_gap = 0, a pool of 2^18 rows, node_limit raised until the record holds at
least 2 * 2^14 + 2049 + 1 childless nodes.  Only the counts matter.  (Seed 1 of that shape proves its optimum
after 29 664 nodes with 20 072 childless records, too few; seed 5 is still open at 45 012 of them, and the first
2^14 + 2051 of its terms hold a leaf whose LP is infeasible, which the first evaluation of a session drops.)"""
from types import SimpleNamespace

import numpy as np
import pytest

from simple_mip_solver_amd import _ffi
from simple_mip_solver_amd.generators import random_dense_milp_arrays
from tests.support import cglp_reference as ref
from tests.support import lp_certificate as cert
from tests.support import tree_reference as tref
from tests.test_restart_gpu import tol   # the project's LP-value-against-HiGHS margin

pytestmark = pytest.mark.gpu
INF = float('inf')

CHUNK = 1 << 14   # mirrors kTrChunk (csrc/treerec_api.hip.h): nodes per launch of a query, a session, a restart
SEG = 2048        # mirrors kSupSeg (csrc/cglp_kernels.hip.h): leaves per workgroup of support_select
MAX_P = _ffi.CGLP_MAX_POINTS   # kSupMaxP
INSTANCE = (64, 32, 5)         # (n, m, seed) of the generator
BATCH = 1024
NEED_CHILDLESS = 2 * CHUNK + (SEG + 1) + 1
T_BIG = CHUNK + SEG + 3        # two chunks, nine full segments and a segment of three leaves
SESSION_T = (SEG - 1, SEG, SEG + 1, 2 * SEG + 5, T_BIG)
POINTS = (1, 16, MAX_P)
EVAL_TOL = 1e-6

_cache = {}


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def close(a, b, rel=1e-9):
    return abs(a - b) <= rel * max(1.0, abs(a), abs(b))


# ---- the tree ---------------------------------------------------------------------------------------------
def grown():
    """The module's one tree, its records and the NumPy reference of every node's bounds.  The counts are
    asserted at every use: a tree that is too small fails the test."""
    if 'tree' not in _cache:
        n, m, seed = INSTANCE
        A, b, c, l, u, ints = random_dense_milp_arrays(n, m, seed=seed)
        ctx = _ffi.default_context()
        p = _ffi.Problem(ctx, A, b, c)
        t = _ffi.Tree(p, ints, l, u, branch_rule='pseudo cost', max_batch=BATCH, pool_capacity=1 << 18)
        t.set_anchor_mode(True)
        t.set_dive(2)
        t.set_tree_record(True)
        limit = 40000
        while True:
            st = t.solve(mip_gap=0.0, frontier_batch=BATCH, node_limit=limit)
            rec = t.tree_records()
            childless = np.flatnonzero((rec['flags'] & _ffi.TR_HAS_CHILDREN) == 0)
            if len(childless) >= NEED_CHILDLESS or st['status'] != 4:
                break
            limit += 10000
        L, U = tref.all_bounds(rec, l, u)
        leaves = childless[rec['lp_status'][childless] != 1]   # the terms a session is opened on, in id order
        _cache['tree'] = SimpleNamespace(n=n, m=m, A=A, b=b, c=c, l=l, u=u, ints=ints, ctx=ctx, p=p, t=t, st=st, rec=rec,
                                         N=len(rec['parent']), childless=childless, leaves=leaves, L=L, U=U)
        print('tree: records', len(rec['parent']), 'childless', len(childless), 'of them not recorded infeasible', len(leaves),
              'recorded infeasible', int((rec['lp_status'] == 1).sum()), 'evaluated', st['evaluated_nodes'], 'status', st['status'])
    g = _cache['tree']
    assert len(g.childless) >= NEED_CHILDLESS, (len(g.childless), NEED_CHILDLESS, g.st)
    assert g.N == g.st['created_nodes'] > 2 * CHUNK
    assert len(g.leaves) >= T_BIG, (len(g.leaves), T_BIG)
    return g


def assert_rows(l, u, L, U, special, what):
    """Every row bit for bit, and the named rows once more by themselves."""
    assert l.shape == L.shape and u.shape == U.shape, what
    bad = np.flatnonzero(np.any(bits(l) != bits(L), axis=1) | np.any(bits(u) != bits(U), axis=1))
    assert len(bad) == 0, (what, 'rows that differ', len(bad), 'the first of them', bad[:8].tolist())
    for k in special:
        assert np.array_equal(bits(l[k]), bits(L[k])) and np.array_equal(bits(u[k]), bits(U[k])), (what, k)


# ---- 1. bounds and re-solve across the chunk edge ------------------------------------------------------------
def test_the_two_bounds_references_agree():
    """all_bounds (one pass down the ids) against lineage_bounds (the walk from the node upwards, first met
    stands), on the deepest nodes and a random sample."""
    g = grown()
    rng = np.random.default_rng(2)
    sample = set(rng.choice(g.N, 300, replace=False).tolist()) | set(np.argsort(g.rec['depth'])[-50:].tolist()) | {0, g.N - 1}
    for i in sorted(sample):
        lo, up = tref.lineage_bounds(g.rec, g.l, g.u, i)
        assert np.array_equal(bits(lo), bits(g.L[i])) and np.array_equal(bits(up), bits(g.U[i])), i


def test_bounds_across_the_chunk_edge():
    g = grown()
    K = CHUNK + 37
    ids = np.random.default_rng(3).integers(0, g.N, K)   # (with repeats, from the whole record)
    before = g.t.tree_record_stats()['materialised']
    l, u = g.t.node_bounds(ids)
    assert g.t.tree_record_stats()['materialised'] - before == K
    assert_rows(l, u, g.L[ids], g.U[ids], (CHUNK - 1, CHUNK, CHUNK + 1, K - 1), 'random ids')
    assert g.N > 2 * CHUNK
    l, u = g.t.node_bounds(np.arange(g.N))
    assert g.t.tree_record_stats()['materialised'] - before == K + g.N
    assert_rows(l, u, g.L, g.U, (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1, g.N - 1), 'the whole tree')


def resolve_ids(g):
    """CHUNK + 37 distinct ids: every recorded-infeasible node (at most half of the list) among recorded-optimal
    ones drawn at random, shuffled."""
    K = CHUNK + 37
    rng = np.random.default_rng(11)
    feasible, infeasible = np.flatnonzero(g.rec['lp_status'] == 0), np.flatnonzero(g.rec['lp_status'] == 1)
    if len(infeasible) > K // 2:
        infeasible = np.sort(rng.choice(infeasible, K // 2, replace=False))
    assert len(feasible) >= K - len(infeasible)
    ids = np.concatenate([rng.choice(feasible, K - len(infeasible), replace=False), infeasible])
    rng.shuffle(ids)
    assert len(ids) == K == len(set(ids.tolist()))
    return ids


def test_resolve_across_the_chunk_edge_is_certified():
    g = grown()
    ids = resolve_ids(g)
    K = len(ids)
    want = g.rec['lp_status'][ids]
    s0 = g.t.tree_record_stats()
    res = g.t.node_solve(ids)
    s1 = g.t.tree_record_stats()
    assert s1['resolved'] - s0['resolved'] == K and s1['materialised'] - s0['materialised'] == K
    wrong = np.flatnonzero(res['status'] != want)
    assert len(wrong) == 0, ('positions whose verdict is not the recorded one', len(wrong), wrong[:8].tolist())
    rng = np.random.default_rng(12)
    pos = np.array(sorted(set(range(CHUNK - 64, min(K, CHUNK + 64))) | set(rng.choice(K, 100, replace=False).tolist())))
    fpos = pos[want[pos] == 0]
    assert np.any(fpos < CHUNK) and np.any(fpos >= CHUNK)
    L, U = g.L[ids], g.U[ids]   # (the NumPy reference, not the kernel's rows)
    Y = np.array([cert.duals_from_basis(g.A, g.c, res['vstat'][k]) for k in fpos])
    M = cert.measure(g.A, g.b, g.c, L[fpos], U[fpos], res['x'][fpos], Y, res['vstat'][fpos])
    for q, k in enumerate(fpos):
        assert close(res['obj'][k], g.rec['objective'][ids[k]]), (k, ids[k], res['obj'][k], g.rec['objective'][ids[k]])
        cert.check_optimal(M, q, float(res['obj'][k]), what=f'position {k} node {ids[k]}')
    proven = 0
    for k in pos[want[pos] == 1][:25]:
        margin, _ = cert.certify_infeasible(g.A, g.b, L[k], U[k], res['vstat'][k])
        assert margin is not None and margin > 0, (k, ids[k])
        proven += 1
    ok = want == 0
    worst = float(np.max(np.abs(res['obj'][ok] - g.rec['objective'][ids[ok]]) / np.maximum(1.0, np.abs(g.rec['objective'][ids[ok]]))))
    print('re-solve: ids', K, 'recorded infeasible among them', int((want == 1).sum()), 'certified optimal', len(fpos),
          'Farkas proofs', proven, 'largest relative distance of an objective from its record', worst)
    _cache['resolve'] = res


def test_resolve_does_not_depend_on_the_chunking():
    """The same ids in calls of at most 1000: the same status and the same bits at every position."""
    g = grown()
    ids = resolve_ids(g)
    K = len(ids)
    whole = _cache['resolve'] if 'resolve' in _cache else g.t.node_solve(ids)
    s0 = g.t.tree_record_stats()
    parts = [g.t.node_solve(ids[k0:k0 + 1000]) for k0 in range(0, K, 1000)]
    s1 = g.t.tree_record_stats()
    assert s1['resolved'] - s0['resolved'] == K and s1['materialised'] - s0['materialised'] == K
    for key in ('status', 'obj', 'x', 'vstat'):
        got = np.concatenate([p[key] for p in parts])
        a, b = (bits(whole[key]), bits(got)) if got.dtype == np.float64 else (whole[key], got)
        differ = np.flatnonzero(np.any((a != b).reshape(K, -1), axis=1))
        assert len(differ) == 0, (key, 'positions that differ', len(differ), 'the first of them', differ[:8].tolist(),
                                  'of them at or above CHUNK', int((differ >= CHUNK).sum()))


# ---- 2. the support session across segments and chunks -------------------------------------------------------
def evaluate(g, ses, pi, pi0, P, all_optimal=True):
    """One evaluation with every check of the output block against the full margins of the same evaluation:
    the rows are the leaves of smallest (margin, node id) among the finite margins in order, each with
    h_t = pi.x_t and x_t in its leaf's box (the NumPy reference's); the head is recomputed from the margins; the
    counters move by the leaves.  A leaf whose LP did not end optimal has margin +inf and is never a row
    (include/mipx_cglp.h); all_optimal: there is none."""
    before = ses.stats()
    res = ses.eval(pi, pi0, tol=EVAL_TOL, max_points=P, want_margins=True)
    after = ses.stats()
    live, m = ses.leaves(), res['margins']
    assert res['leaves'] == len(live) == len(m) == after['leaves']
    finite = np.isfinite(m)
    assert res['not_optimal'] == int((~finite).sum()) and np.all(m[~finite] == INF)
    assert res['not_optimal'] == 0 or not all_optimal, (res['not_optimal'], live[~finite][:8].tolist())
    order = np.lexsort((live, m))
    order = order[finite[order]][:P]
    assert len(res['ids']) == len(order) == min(P, int(finite.sum())) >= 1
    assert np.array_equal(res['ids'], live[order])
    assert np.array_equal(bits(res['h'] - pi0), bits(m[order]))
    assert res['min_margin'] == m.min() and res['min_id'] == live[order[0]]
    assert res['below'] == int((m < -EVAL_TOL).sum())
    assert res['iterations'] >= 0 and res['pivots'] >= 0
    # the first evaluation solves the leaves it was opened on, and the survivors again where any was dropped
    solved = len(live) if before['evaluations'] else before['leaves'] + (len(live) if after['dropped'] else 0)
    assert after['leaf_lps'] - before['leaf_lps'] == solved and after['evaluations'] == before['evaluations'] + 1
    Lr, Ur = g.L[res['ids']], g.U[res['ids']]
    assert np.all(res['x'] >= Lr - 1e-7) and np.all(res['x'] <= Ur + 1e-7)
    assert np.allclose(res['x'] @ pi, res['h'], rtol=0, atol=1e-9 * max(1.0, float(np.abs(res['h']).max())))
    return res, live


def big_session():
    """The largest session, on the first T_BIG terms in id order, after its first evaluation (pi0 = 0: the
    margins are the h_t)."""
    g = grown()
    if 'big' not in _cache:
        opened = g.leaves[:T_BIG]
        ses = g.t.support_open(opened)
        pi = np.random.default_rng(5).uniform(-1, 1, g.n)
        res, live = evaluate(g, ses, pi, 0.0, 16)
        _cache['big'] = SimpleNamespace(ses=ses, opened=opened, pi=pi, res=res, live=live, dropped=ses.leaves(dropped=True))
        print('largest session: opened', len(opened), 'live', len(live), 'dropped', len(_cache['big'].dropped))
    return _cache['big']


def sample_positions(T, seed):
    """Within 2 of every multiple of SEG and of CHUNK, the last three, and 100 at random."""
    pos = set(range(max(T - 3, 0), T)) | set(np.random.default_rng(seed).choice(T, min(100, T), replace=False).tolist())
    for edge in list(range(0, T + 1, SEG)) + [CHUNK]:
        pos |= {k for k in range(edge - 2, edge + 3) if 0 <= k < T}
    return np.array(sorted(pos))


def session_ids(kind, T):
    """'opened': the first T terms of the tree in id order.  'live': the first T of the largest session's
    surviving leaves, so that the selection runs on exactly T leaves whatever the first evaluation drops."""
    return grown().leaves[:T] if kind == 'opened' else big_session().live[:T]


SESSIONS = [('opened', T) for T in SESSION_T] + [('live', T) for T in SESSION_T[:-1]]


@pytest.mark.parametrize('kind,T', SESSIONS, ids=[f'{k} {T}' for k, T in SESSIONS])
def test_selection_is_numpys_over_all_leaves(kind, T):
    g = grown()
    cached = (kind, T) == ('opened', T_BIG)
    ids = session_ids(kind, T)
    assert len(ids) == T
    ses = big_session().ses if cached else g.t.support_open(ids)
    rng = np.random.default_rng(T)
    for P in POINTS:
        res, live = evaluate(g, ses, rng.uniform(-1, 1, g.n), float(rng.uniform(-1, 1)), P)
        if kind == 'live':
            assert len(live) == T and len(ses.leaves(dropped=True)) == 0
    assert sorted(np.concatenate([ses.leaves(), ses.leaves(dropped=True)])) == sorted(ids)
    if cached:
        assert len(ses.leaves()) > CHUNK + 2, 'the second chunk of the packed leaves must not be empty'
    else:
        ses.close()


def check_unit_direction(g, ses, e, warm):
    """pi = e_j: h_t is the leaf's smallest x_j, an integer bound for most leaves -- margins repeat, and the
    (margin, node id) order still decides every row."""
    not_optimal = []
    for P in POINTS:
        res, live = evaluate(g, ses, e, 0.5, P, all_optimal=not warm)
        values, counts = np.unique(res['margins'], return_counts=True)
        assert int(counts[counts > 1].sum()) >= P, (P, len(values))
        selected = res['h'] - 0.5
        assert P == 1 or len(np.unique(selected)) < len(selected), 'no tie among the selected rows'
        not_optimal.append(res['not_optimal'])
    return not_optimal


@pytest.mark.parametrize('kind,T', SESSIONS, ids=[f'{k} {T}' for k, T in SESSIONS])
def test_ties_are_broken_by_node_id(kind, T):
    """pi = 0 (every margin is -pi0), then pi = e_j for the column branched on most often: from the root's basis
    in a session of its own, where every leaf LP ends optimal, and warm-started behind the pi = 0 evaluations.
    The warm start from a basis that is optimal for the zero objective is dual degenerate all the way, and at
    T = 2^14 + 2051 the LP of one leaf of 18 434 (node 18645, position 4701) cycles to the kernel's iteration limit
    (10 600 iterations; so does the CPU oracle on the same LP and basis, and alone in a session of one).  By the
    header such a leaf has margin +inf, counts in block[4] and is never a row: the checks hold it to that."""
    g = grown()
    ids = session_ids(kind, T)
    branched = g.rec['bvar'][g.rec['bvar'] >= 0]
    j = int(np.bincount(branched, minlength=g.n).argmax())   # (every column is integer)
    assert j in g.ints
    e = np.zeros(g.n)
    e[j] = 1.0
    ses = g.t.support_open(ids)
    check_unit_direction(g, ses, e, warm=False)
    ses.close()
    ses = g.t.support_open(ids)
    for P in POINTS:   # pi = 0: the rows are the lowest node ids
        res, live = evaluate(g, ses, np.zeros(g.n), 0.5, P)
        assert np.all(res['margins'] == -0.5)
        assert np.array_equal(res['ids'], np.sort(live)[:P])
        assert res['below'] == res['leaves'] == len(live) and res['min_id'] == live.min()
    not_optimal = check_unit_direction(g, ses, e, warm=True)
    if any(not_optimal):
        print('pi = e_j behind pi = 0: leaf LPs that did not end optimal, per evaluation', not_optimal, 'of', len(ses.leaves()))
    ses.close()


def test_more_points_asked_for_than_there_are_leaves():
    g = grown()
    big = big_session()
    T = len(big.live)
    five = big.live[[T - 1, CHUNK, 0, SEG, CHUNK + 1]]   # (not in id order)
    ses = g.t.support_open(five)
    rng = np.random.default_rng(9)
    for pi in (rng.uniform(-1, 1, g.n), np.zeros(g.n)):
        res, live = evaluate(g, ses, pi, 0.5, 16)
        assert len(res['ids']) == len(res['h']) == len(res['x']) == 5   # (the wrapper cuts the rows at block[3])
        assert sorted(res['ids']) == sorted(five) and np.array_equal(live, five)
    assert np.array_equal(res['ids'], np.sort(five))
    ses.close()


def test_h_is_highs_at_the_segment_and_chunk_edges():
    """h_t of the largest session's first evaluation against HiGHS on the leaf's own LP, the bounds from the NumPy
    reference; allowed: tol(rel=PTOL) of tests/test_restart_gpu.py."""
    g = grown()
    big = big_session()
    T = len(big.live)
    pos = sample_positions(T, 21)
    assert len(pos) <= 250 and {CHUNK - 1, CHUNK, SEG - 1, SEG, T - 1} <= set(pos.tolist())
    h = big.res['margins']   # (pi0 = 0)
    worst = 0.0
    for k in pos:
        i = big.live[k]
        status, want = ref.support(big.pi, g.A, g.b, g.L[i], g.U[i])
        assert status == 0, (k, i, status)
        worst = max(worst, abs(h[k] - want))
        assert abs(h[k] - want) <= tol(h[k], want), (k, i, h[k], want)
    print('h_t against HiGHS:', len(pos), 'leaves, largest deviation', worst)


def test_dropped_leaves_are_the_infeasible_ones():
    g = grown()
    big = big_session()
    assert sorted(np.concatenate([big.live, big.dropped])) == sorted(big.opened)
    assert np.array_equal(big.live, big.opened[~np.isin(big.opened, big.dropped)])   # packed in the order they came in
    zero = np.zeros(g.n)
    for i in big.dropped:
        assert ref.support(zero, g.A, g.b, g.L[i], g.U[i])[0] == 2, ('dropped, but HiGHS finds a point', i)
    for i in np.random.default_rng(22).choice(big.live, 100, replace=False):
        assert ref.support(zero, g.A, g.b, g.L[i], g.U[i])[0] == 0, ('kept, but HiGHS finds no point', i)
    print('largest session dropped', len(big.dropped), 'of', len(big.opened))
    assert len(big.dropped) >= 1


def same_result(a, b):
    assert a.keys() == b.keys()
    for key in a:
        if isinstance(a[key], np.ndarray):
            x, y = (bits(a[key]), bits(b[key])) if a[key].dtype == np.float64 else (a[key], b[key])
            assert x.shape == y.shape and np.array_equal(x, y), key
        else:
            assert a[key] == b[key], (key, a[key], b[key])


def test_margins_do_not_depend_on_the_chunking():
    """Two fresh sessions on the whole large set, evaluated twice each: identical results, and the first the
    cached session's.  A session on the sampled leaves alone (one segment, one chunk): the same margins bit for
    bit, cold and warm-started."""
    g = grown()
    big = big_session()
    pi2 = np.random.default_rng(31).uniform(-1, 1, g.n)
    runs = []
    for _ in range(2):
        ses = g.t.support_open(big.opened)
        r1 = ses.eval(big.pi, 0.0, tol=EVAL_TOL, max_points=16, want_margins=True)
        r2 = ses.eval(pi2, 0.25, tol=EVAL_TOL, max_points=MAX_P, want_margins=True)
        assert np.array_equal(ses.leaves(), big.live) and np.array_equal(ses.leaves(dropped=True), big.dropped)
        ses.close()
        runs.append((r1, r2))
    same_result(runs[0][0], runs[1][0])
    same_result(runs[0][1], runs[1][1])
    same_result(runs[0][0], big.res)
    pos = sample_positions(len(big.live), 21)
    small = g.t.support_open(big.live[pos])
    assert len(pos) <= SEG
    s1 = small.eval(big.pi, 0.0, tol=EVAL_TOL, max_points=16, want_margins=True)
    s2 = small.eval(pi2, 0.25, tol=EVAL_TOL, max_points=MAX_P, want_margins=True)
    assert np.array_equal(small.leaves(), big.live[pos])
    small.close()
    for name, s, r in (('from the root basis', s1, runs[0][0]), ('warm-started', s2, runs[0][1])):
        differ = np.flatnonzero(bits(s['margins']) != bits(r['margins'][pos]))
        assert len(differ) == 0, (name, 'positions of the large session that differ', pos[differ][:8].tolist())


# ---- 3. a restart with more than one chunk of seeds ----------------------------------------------------------
def test_restart_seeds_past_one_chunk():
    g = grown()
    assert len(g.childless) > 2 * CHUNK
    p2 = _ffi.Problem(g.ctx, g.A, g.b + np.random.default_rng(1).uniform(-2, 2, g.m), g.c)
    t = _ffi.Tree.restart(g.t, p2)
    try:
        seeds = t.restart_seeds()
        assert np.array_equal(seeds, g.childless)
        S = len(seeds)
        stats = t.restart_stats()
        assert stats['skeleton'] == g.N and stats['seeds'] == S
        assert stats['device_bytes'] == S * (16 * g.n + g.n + g.m) and stats['seed_ms'] > 0
        first = t.stats()
        assert first['open_nodes'] == S and first['created_nodes'] == g.N and first['evaluated_nodes'] == 0
        # best first: the seeds sit in the queue in id order, all keyed -inf
        L, U, V, db = t.peek_open(S)
        assert_rows(L, U, g.L[seeds], g.U[seeds], (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK, S - 1), 'seed rows')
        assert np.all(db == -INF)
        assert np.all(V == V[:1]) and int(np.sum(V[0] == cert.BASIC)) == g.m
        st = t.solve(mip_gap=1e-9, frontier_batch=BATCH, max_steps=2)
        assert st['evaluated_nodes'] >= 1 and st['steps'] <= 2 and st['status'] in (1, 2, 4), st
    finally:
        t.close()
        p2.close()
