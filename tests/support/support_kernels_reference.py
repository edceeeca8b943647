"""The kernels behind a support evaluation, restated in NumPy from the words of include/mipx_supportkernels.h,
include/mipx_cglp.h and include/mipx_cglp_screen.h (test infrastructure only): the selection, the packing, the gather,
the scatter, the mark, and one evaluation chained the way mipx_tree_support_eval_ex chains them, with the leaf LPs'
results an argument.  Every function writes into buffers the caller filled with FILL, and writes only what the headers
say the kernels write, so that a comparison of whole buffers also holds what must stay untouched.  Nothing here uses
the engine, and nothing gets a tolerance.

The selection is stated WITHOUT np.lexsort (two stable sorts per segment, a heap over all leaves for the merge), so
that tests/test_support_kernels_abi.py can hold it against np.lexsort; the pack is stated position by position in
cumulative sums and held against np.flatnonzero."""
import functools
import heapq

import numpy as np

from tests.support import cglp_screen_reference as screen_ref

FILL = 0x5a
SEG = 2048                 # positions per segment
HEAD = 8                   # doubles in front of the rows of the block
NONE = 0x7fffffff          # the node id of "no leaf"
MAX_P = 1024
MAX_ID = NONE - 1
I32_MAX = 2 ** 31 - 1
INF = float('inf')


def filled(shape, dtype):
    a = np.empty(shape, dtype)
    a.view(np.uint8).reshape(-1)[:] = FILL
    return a


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def untouched(a):
    return bool(np.all(np.ascontiguousarray(a).view(np.uint8) == FILL))


def segments(T):
    return (T + SEG - 1) // SEG


# ---- select -------------------------------------------------------------------------------------------------------------
def ok_leaves(c):
    return (np.asarray(c['status']) == 0) & ~np.isnan(c['obj'])


def margins(c):
    with np.errstate(invalid='ignore'):
        return np.where(ok_leaves(c), c['obj'] - c['pi0'], INF)


def _ascending(mg, ids, pos):
    """pos in ascending order of (mg[pos], ids[pos]): a stable sort by id, then a stable sort by margin."""
    pos = pos[np.argsort(ids[pos], kind='stable')]
    return pos[np.argsort(mg[pos], kind='stable')]


def select_buffers(c):
    T, n, P, G = c['T'], c['n'], c['P'], segments(c['T'])
    return dict(margin=filled(T, np.float64), cand_m=filled((G, P), np.float64), cand_id=filled((G, P), np.int32),
                cand_t=filled((G, P), np.int32), seg_sum=filled((G, 4), np.float64), block=filled(HEAD + P * (n + 2), np.float64))


def select(c, out):
    """What support_select and support_select_merge write, into out (select_buffers)."""
    T, n, P = c['T'], c['n'], c['P']
    if T == 0:
        return out
    ok, mg, ids = ok_leaves(c), margins(c), np.asarray(c['ids'], np.int64)
    out['margin'][:] = mg
    below = ok & (mg < -c['tol'])
    for g in range(segments(T)):
        lo, hi = g * SEG, min(T, (g + 1) * SEG)
        pos = _ascending(mg, ids, lo + np.flatnonzero(ok[lo:hi]))[:P]
        k = len(pos)
        out['cand_m'][g, :k], out['cand_id'][g, :k], out['cand_t'][g, :k] = mg[pos], ids[pos], pos
        out['cand_m'][g, k:], out['cand_id'][g, k:], out['cand_t'][g, k:] = INF, NONE, -1
        out['seg_sum'][g] = [below[lo:hi].sum(), (~ok[lo:hi]).sum(), float(np.asarray(c['iters'][lo:hi], np.int64).sum()),
                             float(np.asarray(c['npivots'][lo:hi], np.int64).sum())]
    where = np.flatnonzero(ok)
    best = heapq.nsmallest(P, zip(mg[where].tolist(), ids[where].tolist(), where.tolist()))
    nsel = len(best)
    block = out['block']
    block[:HEAD] = [best[0][0] if nsel else INF, best[0][1] if nsel else -1, below.sum(), nsel, (~ok).sum(),
                    float(np.asarray(c['iters'], np.int64).sum()), float(np.asarray(c['npivots'], np.int64).sum()), T]
    rows = block[HEAD:].reshape(P, n + 2)
    x = np.asarray(c['x'], np.float64).reshape(T, n)
    for p, (_, node, t) in enumerate(best):
        rows[p, 0], rows[p, 1], rows[p, 2:] = node, c['obj'][t], x[t]
    return out


# ---- pack ----------------------------------------------------------------------------------------------------------------
def pack_buffers(T):
    G = segments(T)
    return dict(seg_count=filled(G, np.int32), seg_min=filled(G, np.float64), packed=filled(T, np.int32),
                count=filled(1, np.int32), min_margin=filled(1, np.float64))


def takes(mode, skip, status):
    return np.asarray(status) != 0 if mode else np.asarray(skip) == 0


def pack(T, mode, pi0, skip, status, bound, out):
    """What support_pack_count and support_pack write, into out (pack_buffers)."""
    if T == 0:
        return out
    take = takes(mode, skip, status)
    rank = np.cumsum(take) - take                     # how many taken positions lie before each position
    for t in range(T) if T <= 64 else ():             # (the small sizes position by position, as the words say it)
        if take[t]:
            out['packed'][rank[t]] = t
    if T > 64:
        out['packed'][rank[take]] = np.arange(T, dtype=np.int32)[take]
    out['count'][0] = int(take.sum())
    with_margin = mode == 0 and bound is not None
    for g in range(segments(T)):
        lo, hi = g * SEG, min(T, (g + 1) * SEG)
        out['seg_count'][g] = int(take[lo:hi].sum())
        left = ~take[lo:hi]
        out['seg_min'][g] = (np.asarray(bound, np.float64)[lo:hi][left] - pi0).min() if with_margin and left.any() else INF
    out['min_margin'][0] = out['seg_min'].min()
    return out


# ---- gather, scatter, mark -----------------------------------------------------------------------------------------------
LEAF_KEYS = ('x', 'obj', 'y', 'v', 'status', 'iters', 'npivots', 'has_y')


def gather(count, packed, l, u, v, pl, pu, pv_in):
    """Rows packed[k] of l, u and (if v is given) v into rows k of pl, pu, pv_in."""
    for k in range(count):
        t = packed[k]
        pl[k], pu[k] = l[t], u[t]
        if v is not None:
            pv_in[k] = v[t]


def scatter(count, packed, add, lp, leaf):
    """lp: the packed-side results (px, pobj, py, pv_out, pstatus, piters, pnpivots); leaf: the leaf-side arrays
    LEAF_KEYS, written in place.  A failed LP keeps the leaf's duals and its has_y."""
    for k in range(count):
        t = packed[k]
        leaf['x'][t], leaf['v'][t] = lp['px'][k], lp['pv_out'][k]
        leaf['obj'][t], leaf['status'][t] = lp['pobj'][k], lp['pstatus'][k]
        with np.errstate(over='ignore'):   # (int32 wraps as the kernel's int does; the cases stay below 2^31)
            leaf['iters'][t] = (leaf['iters'][t] if add else 0) + lp['piters'][k]
            leaf['npivots'][t] = (leaf['npivots'][t] if add else 0) + lp['pnpivots'][k]
        if lp['pstatus'][k] == 0:
            leaf['y'][t] = lp['py'][k]
            leaf['has_y'][t] = 1


def mark(T, status, has_y):
    has_y[:T] = np.asarray(status[:T]) == 0


# ---- one evaluation ------------------------------------------------------------------------------------------------------
def screen_record(leaf, bound, screened):
    """What a session's screen leaves in the record of a screened leaf (csrc: the four pointers mipx_support_screen_batch
    does not pass, so the chain applies them on the host): the bound in the place of h_t, optimal, no iterations."""
    s = np.asarray(screened) != 0
    leaf['obj'][s], leaf['status'][s], leaf['iters'][s], leaf['npivots'][s] = np.asarray(bound)[s], 0, 0, 0


def lp_rows(lp, packed, count):
    """The packed-side results of a launch over packed[:count]: the rows of per-leaf results lp (keyed like scatter's)."""
    sel = np.asarray(packed[:count], np.int64)
    return {k: np.ascontiguousarray(a[sel]) for k, a in lp.items()}


def evaluation(A, b, pi, pi0, tol, screen_tol, P, ids, l, u, leaf, lp1, lp2):
    """A screening evaluation with the cold retry, step by step: screen -> pack by skip -> gather warm -> scatter -> pack by
    status -> gather cold -> scatter with add -> select.  leaf (LEAF_KEYS) is written in place; lp1, lp2: the results
    of the two launches per LEAF position (a launch reads the rows of its packed leaves).  Returns every intermediate."""
    T, n = l.shape
    m = leaf['y'].shape[1]
    steps = {}
    scr = screen_ref.screen(A, b, pi, pi0, screen_tol, l, u, leaf['y'], leaf['has_y'])
    steps['screen'] = scr
    screen_record(leaf, scr['bound'], scr['screened'])
    p1 = pack(T, 0, pi0, scr['screened'], None, scr['bound'], pack_buffers(T))
    steps['pack1'] = p1
    c1 = int(p1['count'][0])
    g1 = dict(pl=filled((T, n), np.float64), pu=filled((T, n), np.float64), pv_in=filled((T, n + m), np.int8))
    gather(c1, p1['packed'], l, u, leaf['v'], **g1)
    steps['gather1'] = g1
    scatter(c1, p1['packed'], 0, lp_rows(lp1, p1['packed'], c1), leaf)
    steps['leaf1'] = {k: leaf[k].copy() for k in LEAF_KEYS}
    p2 = pack(T, 1, pi0, None, leaf['status'], None, pack_buffers(T))
    steps['pack2'] = p2
    c2 = int(p2['count'][0])
    g2 = dict(pl=filled((T, n), np.float64), pu=filled((T, n), np.float64), pv_in=filled((T, n + m), np.int8))
    gather(c2, p2['packed'], l, u, None, **g2)
    steps['gather2'] = g2
    rows2 = lp_rows(lp2, p2['packed'], c2)
    scatter(c2, p2['packed'], 1, rows2, leaf)
    steps['leaf2'] = {k: leaf[k].copy() for k in LEAF_KEYS}
    steps['retried'], steps['retried_ok'] = c2, int((rows2['pstatus'] == 0).sum())
    c = dict(T=T, n=n, P=P, pi0=pi0, tol=tol, ids=ids, status=leaf['status'], obj=leaf['obj'], x=leaf['x'], iters=leaf['iters'],
             npivots=leaf['npivots'])
    steps['select_case'] = c
    steps['select'] = select(c, select_buffers(c))
    return steps


# ---- the cases -----------------------------------------------------------------------------------------------------------
SIZES = (1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097, 3 * SEG + 5)
# 66 segments: wave 0 of a 256-thread sum over the segments no longer holds them all (65, the first such number: T_65);
# 258 segments: a thread takes two
T_65, T_WAVES, T_TWICE = 64 * SEG + 1, 65 * SEG + 3, 257 * SEG + 3
ROWS_ASKED = (1, 2, 16, 1023, 1024)
WIDTHS = (1, 2, 255, 256, 257, 1024)
CONTENTS = ('mixed', 'ties', 'empty-segment', 'none-ok', 'few-ok', 'tol-edge', 'big-counts')


def _ids(rng, T):
    """T distinct ids out of 0 .. 2^31 - 2 in no order of position, 0 and 2^31 - 2 among them where there is room."""
    ids = np.unique(rng.integers(0, MAX_ID + 1, 2 * T + 8))
    ids = ids[(ids != 0) & (ids != MAX_ID)]
    ids = rng.permutation(ids)[:T]
    if T >= 2:
        ids[rng.integers(0, T)] = 0
        ids[(int(np.flatnonzero(ids == 0)[0]) + 1 + rng.integers(0, T - 1)) % T] = MAX_ID
    return ids.astype(np.int64)


@functools.lru_cache(maxsize=None)
def select_case(content, T, n, P, seed=0):
    """A selection case and the count of every kind of leaf in it (`kinds`).  The arrays must be left as they are."""
    rng = np.random.default_rng([CONTENTS.index(content), T, n, P, seed])
    ids = _ids(rng, T)
    status = np.zeros(T, np.int32)
    obj = rng.integers(-6, 7, T) * 0.25                                   # few values: most margins tie, ids decide
    iters, npivots = rng.integers(0, 50, T).astype(np.int32), rng.integers(0, 9, T).astype(np.int32)
    pi0, tol = 0.375, 0.25
    if content in ('mixed', 'empty-segment', 'few-ok', 'big-counts'):
        bad = rng.random(T) < 0.15
        status[bad] = rng.integers(1, 4, int(bad.sum()))
        odd = rng.random(T)
        obj[odd < 0.03] = np.nan
        obj[(odd >= 0.03) & (odd < 0.05)] = INF
        obj[(odd >= 0.05) & (odd < 0.07)] = -INF
        if T >= 64 and content != 'few-ok':   # one of each kind whatever was drawn, all in the first segment
            spots = rng.permutation(min(T, SEG))[:4]
            status[spots] = [0, 0, 0, 3]
            obj[spots[:3]] = [np.nan, INF, -INF]
    if content == 'ties':               # one margin everywhere, ids descending along the positions: every choice is the ids'
        obj[:] = 0.5
        ids = np.sort(ids)[::-1].copy()
        if T > 8:
            obj[rng.integers(0, T, T // 8)] = -0.0                          # ... and -0.0 against +0.0 at pi0 = 0
            obj[rng.integers(0, T, T // 8)] = 0.0
        pi0 = 0.0
    if content == 'empty-segment' and T > SEG:
        status[SEG:min(T, 2 * SEG)] = 2
    if content == 'none-ok':
        status[:] = rng.integers(1, 4, T)
        status[::3] = 0
        obj[::3] = np.nan
    if content == 'few-ok':             # fewer ok leaves than P: in the first segment, and (P > 3) overall
        keep = max(1, min(P, T) // 2) if P > 3 else 1
        first = rng.permutation(min(T, SEG))[keep:]
        status[first] = 1
        if P > 3:
            rest = SEG + rng.permutation(max(0, T - SEG))[keep // 2:]
            status[rest] = 3
    if content == 'tol-edge':           # pi0 = 0: the margin is the objective, exactly
        pi0, tol = 0.0, 0.5
        obj[rng.random(T) < 0.3] = -0.5
        obj[rng.random(T) < 0.3] = np.nextafter(-0.5, -INF)
    if content == 'big-counts':
        big = rng.random(T) < 0.5
        iters[big], npivots[big] = I32_MAX, I32_MAX - rng.integers(0, 3, int(big.sum()))
    x = rng.standard_normal((T, n)).round(3)
    c = dict(content=content, T=T, n=n, P=P, pi0=pi0, tol=tol, ids=ids, status=status, obj=obj, x=x, iters=iters, npivots=npivots)
    c['kinds'] = kinds(c)
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def kinds(c):
    """How many leaves (or segments) of each kind a case holds: the tests print and hold these."""
    ok, mg, T, P = ok_leaves(c), margins(c), c['T'], c['P']
    seg_ok = [int(ok[g * SEG:(g + 1) * SEG].sum()) for g in range(segments(T))]
    okm, oki = mg[ok], np.asarray(c['ids'])[ok]
    order = np.argsort(okm, kind='stable')
    srt = okm[order]
    tie_pairs = int((srt[1:] == srt[:-1]).sum())
    pos = np.flatnonzero(ok)
    same = {}
    for t, v in zip(pos.tolist(), okm.tolist()):
        same.setdefault(v, []).append(t)
    span = sum(1 for ts in same.values() if ts[0] // SEG != ts[-1] // SEG)
    desc = sum(1 for ts in same.values() if any(c['ids'][a] > c['ids'][b] for a, b in zip(ts, ts[1:])))
    with np.errstate(invalid='ignore'):
        return dict(ok=int(ok.sum()), status_bad=int((c['status'] != 0).sum()), nan=int((np.isnan(c['obj']) & (c['status'] == 0)).sum()),
                    pos_inf=int(((c['obj'] == INF) & (c['status'] == 0)).sum()), neg_inf=int(((c['obj'] == -INF) & (c['status'] == 0)).sum()),
                    tie_pairs=tie_pairs, ties_across_segments=span, ties_descending_ids=desc,
                    ids_unordered=int((np.diff(c['ids']) < 0).sum()), max_id=int(np.max(c['ids'])),
                    empty_segments=sum(1 for s in seg_ok if s == 0), short_segments=sum(1 for s in seg_ok if 0 < s < P),
                    short_overall=int(ok.sum() < P), at_tol=int((ok & (mg == -c['tol'])).sum()),
                    just_below_tol=int((ok & (mg == np.nextafter(-c['tol'], -INF))).sum()),
                    iters_total=int(np.asarray(c['iters'], np.int64).sum()), pivots_total=int(np.asarray(c['npivots'], np.int64).sum()),
                    neg_zero=int((ok & (mg == 0) & np.signbit(mg)).sum()))


# pack: which leaves are taken
DENSITIES = ('none', 'all', 'half', 'first', 'last', 'first-of-segment', 'last-of-segment', 'empty-middle-segment')
MARGIN_SPOTS = ('last-segment', 'first-segment', 'last-item-of-a-thread', 'absent')


@functools.lru_cache(maxsize=None)
def pack_case(density, T, spot='last-segment'):
    """take (T bools), and a bound whose smallest entry over the leaves NOT taken sits where `spot` says."""
    rng = np.random.default_rng([DENSITIES.index(density), T, MARGIN_SPOTS.index(spot)])
    G = segments(T)
    take = np.zeros(T, bool)
    if density == 'all':
        take[:] = True
    elif density in ('half', 'empty-middle-segment'):
        take = rng.random(T) < 0.5
        if density == 'empty-middle-segment' and G >= 3:
            take[(G // 2) * SEG:(G // 2 + 1) * SEG] = False
    elif density == 'first':
        take[0] = True
    elif density == 'last':
        take[T - 1] = True
    elif density == 'first-of-segment':
        take[(G - 1) * SEG if (G - 1) * SEG < T else 0] = True
    elif density == 'last-of-segment':
        take[min(T, SEG * max(1, G - 1)) - 1] = True
    bound = rng.integers(0, 1000, T) * 0.125                      # ties among the skipped: a minimum is a minimum
    at = -1
    if spot == 'absent':
        take = np.ones(T, bool)
    elif density in ('half', 'empty-middle-segment') and T > 16:   # the spot is a skipped leaf, whatever was drawn there
        at = {'last-segment': T - 1, 'first-segment': 5, 'last-item-of-a-thread': (T // 2) // 8 * 8 + 7}[spot]
        take[at] = False
        bound[at] = -7.625
    elif not take.all():
        at = int(np.flatnonzero(~take)[-1])
        bound[at] = -7.625
    bound[take] = -1e9                                             # the taken leaves' bounds must not count
    skip = (~take).astype(np.uint8)
    status = np.where(take, rng.integers(1, 4, T), 0).astype(np.int32)
    for a in (skip, status, bound):
        a.setflags(write=False)
    return dict(T=T, take=take, skip=skip, status=status, bound=bound, at=at, pi0=0.5)


# gather / scatter / mark
MOVE_SHAPES = ((1, 0), (1, 1), (5, 3), (255, 1), (256, 0), (257, 255), (1024, 1024))
MOVE_LEAVES = (1, 5, 300)


def move_counts(T):
    return sorted({0, 1, T, max(1, T // 2)})


@functools.lru_cache(maxsize=None)
def move_case(n, m, T, count):
    """Leaf-side and packed-side arrays of a gather and a scatter: `count` ascending positions out of T; verdicts mixed;
    has_y 0 and 1 beforehand under both verdicts where there is room for all four."""
    rng = np.random.default_rng([n, m, T, count])
    packed = np.sort(rng.permutation(T)[:count]).astype(np.int32)
    leaf = dict(l=rng.standard_normal((T, n)), u=rng.standard_normal((T, n)), x=rng.standard_normal((T, n)), obj=rng.standard_normal(T),
                y=rng.standard_normal((T, m)), v=rng.integers(-1, 3, (T, n + m)).astype(np.int8),
                status=rng.integers(0, 4, T).astype(np.int32), iters=rng.integers(0, 1000, T).astype(np.int32),
                npivots=rng.integers(0, 100, T).astype(np.int32), has_y=(rng.random(T) < 0.5).astype(np.uint8))
    lp = dict(px=rng.standard_normal((count, n)), pobj=rng.standard_normal(count), py=rng.standard_normal((count, m)),
              pv_out=rng.integers(-1, 3, (count, n + m)).astype(np.int8), pstatus=(rng.integers(0, 4, count) * (rng.random(count) < 0.5)).astype(np.int32),
              piters=rng.integers(0, 1000, count).astype(np.int32), pnpivots=rng.integers(0, 100, count).astype(np.int32))
    if count >= 4:   # all four of (had duals or not) x (fails or not)
        lp['pstatus'][:4] = [0, 0, 2, 3]
        leaf['has_y'][packed[:4]] = [0, 1, 0, 1]
    for a in list(leaf.values()) + list(lp.values()) + [packed]:
        a.setflags(write=False)
    return dict(n=n, m=m, T=T, count=count, packed=packed, leaf=leaf, lp=lp)
