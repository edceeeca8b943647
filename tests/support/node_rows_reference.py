"""The kernels that move node rows (make_children, pack_nodes, unpack_nodes, gather_plain_nodes, treerec_bounds,
restart_seed, the cutmig_* and spill_* kernels), restated in plain NumPy from their headers, and the named synthetic
cases the tests compare them on (tests/test_node_rows_abi.py without a GPU, tests/test_node_rows_gpu.py against the
device through include/mipx_noderows.h).  Test infrastructure only: no product code is imported.

Every comparison is of bits.  The only arithmetic is floor and ceil, which are exact; doubles are compared as uint64 views,
so that -0.0, infinities and NaN payloads count.  An array the kernels write starts as bytes 0x5a (filled): whatever a
restatement does not write stays the sentinel, and so must whatever the kernel does not write.

  children  the child row is the parent's pool row with one bound replaced, u[var] = floor(x) for the left child and
            l[var] = ceil(x) for the right; the parent's n + m + kcut codes (and kcut ids, and ncut) are copied.
  message   row k of the message is [l (n f64) | u (n f64) | nvs codes | pad to 8 bytes]; the pad is never written.
  lineage   (a) walk(): the kernel's walk, node up to root, the first branching met per (column, side) stands;
            (b) descend(): the search's own order, root down to the node, every branching overwriting the bound.
            Both follow the mirror as the kernel does: the walk ends at id 0, at an id outside the mirror, and at a parent
            that is not below its child; an entry whose variable is outside 0 .. n-1 is passed over.
  cutmig    lists: [ncut, ids (0 past ncut)];  gather: table row r = store row src[r];  scatter: store row base + r =
            table row r;  unpack_lists: ids = base + ref in list order, a list that does not fit gives ncut = 0, untouched
            ids and one count in bad.
  spill     the record layout of include/mipx_spill.h (encode / decode); offsets are the exclusive prefix sums.
"""
import functools
import re

import numpy as np

INF = float('inf')
FILL = 0x5a
WIDTHS_256 = (1, 2, 255, 256, 257, 511, 513, 1024)    # block-per-row kernels step by 256
WIDTHS_64 = (1, 63, 64, 65, 129, 1024)                # wave-per-row kernels step by 64
LINEAGE_CHUNK = 1 << 14                               # kTrChunk: ids per launch of the lineage kernels
BRANCH_VALUES = (2.5, 3.0, -1.5, -0.5, 0.0, 1e15 + 0.5)
NAN_PAYLOAD = np.array([0x7ff8_0000_dead_beef], np.uint64).view(np.float64)[0]
SPECIALS = np.array([INF, -INF, 0.0, -0.0, 1.0, -1.0, 2.5, 1e300, NAN_PAYLOAD])


def filled(shape, dtype):
    a = np.empty(shape, dtype)
    a.view(np.uint8).fill(FILL) if a.size else None
    return a


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def pad8(b):
    return b + bytes((-len(b)) % 8)


def rows_of(rng, rows, n):
    """rows x n doubles: normals mixed with the specials (a NaN with a payload among them)."""
    a = rng.normal(size=(rows, n)) * 10.0
    pick = rng.random((rows, n)) < 0.3
    a[pick] = rng.choice(SPECIALS, int(pick.sum()))
    return a


def scattered_slots(rng, count, rows):
    """count distinct rows of a pool of `rows`, unordered, with gaps, row 0 and the last row among them (count >= 2)."""
    assert rows > count
    if count == 1:
        return np.array([rows - 1], np.int32)
    mid = rng.choice(np.arange(1, rows - 1), count - 2, replace=False)
    s = np.concatenate([[rows - 1], mid, [0]]).astype(np.int32)
    if count > 3:
        s[1:-1] = s[1:-1][np.argsort(-s[1:-1].astype(np.int64) % 7, kind='stable')]
    return s


# ---- children ------------------------------------------------------------------------------------------------------------
def children_restated(c):
    n, m, cut = c['n'], c['m'], c['mstride'] > 0
    out = {k: c[k].copy() for k in ('dst_l', 'dst_u', 'dst_v')}
    if cut:
        out['dst_ncut'], out['dst_ids'] = c['dst_ncut'].copy(), c['dst_ids'].copy()
    for p in range(len(c['var'])):
        ps, pos, j = int(c['parent_slot'][p]), int(c['parent_pos'][p]), int(c['var'][p])
        xv = c['x'][pos, j]
        kcut = int(c['src_ncut'][pos]) if cut else 0
        for right in (0, 1):
            ds = int(c['child_slot'][2 * p + right])
            lo, up = c['src_l'][ps].copy(), c['src_u'][ps].copy()
            if right:
                lo[j] = np.ceil(xv)
            else:
                up[j] = np.floor(xv)
            out['dst_l'][ds], out['dst_u'][ds] = lo, up
            out['dst_v'][ds, :n + m + kcut] = c['vstat'][pos, :n + m + kcut]
            if cut:
                out['dst_ncut'][ds] = kcut
                out['dst_ids'][ds, :kcut] = c['src_ids'][pos, :kcut]
    return out


def _children_case(n, m, seed, kc=0, mstride=0, kcuts=()):
    rng = np.random.default_rng(seed)
    cut = mstride > 0
    stride = mstride if cut else m
    src_rows, batch_rows = 5, 6
    vars_ = sorted({v for v in (0, 255, 256, n - 1) if 0 <= v < n})
    count = max(len(BRANCH_VALUES), 2 * len(vars_), len(kcuts))
    var = np.array([vars_[p % len(vars_)] for p in range(count)], np.int32)
    parent_slot = np.array([(4, 0, 2)[p % 3] for p in range(count)], np.int32)       # unordered, rows 0 and last
    parent_slot[:len(vars_)] = 4                                                     # one parent, several variables
    parent_pos = np.array([p % 5 for p in range(count)], np.int32)                   # (every (pos, var) is one pair's)
    parent_pos[:len(vars_)] = 5
    src_l, src_u = rows_of(rng, src_rows, n), rows_of(rng, src_rows, n)
    x = rng.normal(size=(batch_rows, n)) * 7.0
    for p in range(count):
        x[parent_pos[p], var[p]] = BRANCH_VALUES[p % len(BRANCH_VALUES)]
    src_l[4, var[0]], src_u[4, var[0]] = -INF, INF            # a branched column whose parent bound is infinite
    if n > 1:
        free = [j for j in range(n) if j not in vars_]
        if free:
            src_l[4, free[0]] = -0.0                          # -0.0 in a column that is not branched on
            src_u[0, free[-1]] = -0.0
    vstat = rng.integers(-3, 6, (batch_rows, n + stride)).astype(np.int8)
    dst_rows = 2 * count + 3
    child_slot = scattered_slots(rng, 2 * count, dst_rows)
    c = dict(n=n, m=m, mstride=mstride, kc=kc, src_l=src_l, src_u=src_u, x=x, vstat=vstat, parent_slot=parent_slot,
             parent_pos=parent_pos, var=var, child_slot=child_slot, dst_l=filled((dst_rows, n), np.float64),
             dst_u=filled((dst_rows, n), np.float64), dst_v=filled((dst_rows, n + stride), np.int8),
             src_ncut=None, src_ids=None, dst_ncut=None, dst_ids=None)
    if cut:
        ncut = np.array([kcuts[r % len(kcuts)] for r in range(batch_rows)], np.int32)
        c.update(src_ncut=ncut, src_ids=rng.integers(0, 1 << 20, (batch_rows, kc)).astype(np.int32),
                 dst_ncut=filled(dst_rows, np.int32), dst_ids=filled((dst_rows, kc), np.int32))
    return c


CHILDREN_PLAIN = {'children-n%d-m%d' % (n, m): (n, m) for n, m in
                  ((1, 1), (2, 3), (255, 2), (256, 1), (257, 8), (511, 300), (513, 2), (1024, 1023))}
CHILDREN_CUT = {'children-cut-kc64-loose': dict(n=257, m=3, kc=64, mstride=3 + 64, kcuts=(0, 1, 63, 64)),
                'children-cut-kc1-tight': dict(n=5, m=4, kc=1, mstride=4 + 1, kcuts=(1, 0)),
                'children-cut-kc63-tight': dict(n=5, m=4, kc=63, mstride=4 + 63, kcuts=(63,)),
                'children-cut-kc64-tight': dict(n=300, m=250, kc=64, mstride=250 + 64, kcuts=(64, 0)),
                'children-cut-kc0': dict(n=5, m=4, kc=0, mstride=4, kcuts=(0,))}
CHILDREN_CASES = list(CHILDREN_PLAIN) + list(CHILDREN_CUT)


# ---- message -------------------------------------------------------------------------------------------------------------
def rowbytes(n, nvs):
    return (16 * n + nvs + 7) // 8 * 8


def message_packed(n, nvs, slot, pool_l, pool_u, pool_v, msg):
    """msg (count x rowbytes uint8) after pack_nodes: the pad bytes stay."""
    out = msg.copy().reshape(len(slot), rowbytes(n, nvs))
    for k, s in enumerate(slot):
        row = pool_l[s].tobytes() + pool_u[s].tobytes() + pool_v[s].tobytes()
        out[k, :len(row)] = np.frombuffer(row, np.uint8)
    return out


def message_unpacked(n, nvs, slot, msg, pool_l, pool_u, pool_v):
    l, u, v = pool_l.copy(), pool_u.copy(), pool_v.copy()
    msg = np.ascontiguousarray(msg).reshape(len(slot), rowbytes(n, nvs))
    for k, s in enumerate(slot):
        l[s] = msg[k, :8 * n].view(np.float64)
        u[s] = msg[k, 8 * n:16 * n].view(np.float64)
        v[s] = msg[k, 16 * n:16 * n + nvs].view(np.int8)
    return l, u, v


def _message_case(n, nvs, count, seed):
    rng = np.random.default_rng(seed)
    rows = count + 4
    other = scattered_slots(rng, count, rows + 2)
    other[:2] = other[1::-1]                                      # (another order than slot's, still not ascending)
    return dict(n=n, nvs=nvs, slot=scattered_slots(rng, count, rows), other=other,
                pool_l=rows_of(rng, rows, n), pool_u=rows_of(rng, rows, n),
                pool_v=rng.integers(-3, 6, (rows, nvs)).astype(np.int8))


# (n, nvs): every width; nvs % 8 in {0, 1, 7}; nv odd and even, above 256 and above 1024
MESSAGE_SHAPES = ((1, 2), (2, 7), (255, 257), (256, 264), (257, 258), (511, 519), (513, 520), (1024, 2047))
MESSAGE_CASES = ['message-n%d-nvs%d' % s for s in MESSAGE_SHAPES]
# gather_plain_nodes: (n, m, nvs_pool)
GATHER_SHAPES = ((1, 1, 2), (2, 3, 6), (255, 2, 321), (256, 1, 257), (257, 8, 329), (511, 300, 875), (513, 2, 515), (1024, 1023, 2111))
GATHER_CASES = ['gather-n%d-m%d-pool%d' % s for s in GATHER_SHAPES]


def gather_plain_restated(c):
    l, u, v = c['l'].copy(), c['u'].copy(), c['v'].copy()
    for k, s in enumerate(c['slot']):
        l[k], u[k], v[k] = c['pool_l'][s], c['pool_u'][s], c['pool_v'][s, :c['n'] + c['m']]
    return l, u, v


# ---- lineage -------------------------------------------------------------------------------------------------------------
def path_up(parent, node):
    """The ids the kernel's walk visits from `node`, in its order (the root, id 0, is never visited)."""
    N, out, i = len(parent), [], int(node)
    while 0 < i < N:
        out.append(i)
        i = int(parent[i]) if parent[i] < i else -1
    return out


def _branch(vd, val, n):
    var, right = int(vd) >> 1, int(vd) & 1
    return (var, right, np.ceil(val) if right else np.floor(val)) if 0 <= var < n else None


def walk(parent, vd, val, node, root_l, root_u):
    """(a) node up to root: the first branching met per (column, side) stands."""
    lo, up, seen = root_l.copy(), root_u.copy(), set()
    for i in path_up(parent, node):
        b = _branch(vd[i], val[i], len(lo))
        if b is not None and b[:2] not in seen:
            seen.add(b[:2])
            (lo if b[1] else up)[b[0]] = b[2]
    return lo, up


def descend(parent, vd, val, node, root_l, root_u):
    """(b) root down to the node: every branching overwrites the bound, as the search did when it built the tree."""
    lo, up = root_l.copy(), root_u.copy()
    for i in reversed(path_up(parent, node)):
        b = _branch(vd[i], val[i], len(lo))
        if b is not None:
            (lo if b[1] else up)[b[0]] = b[2]
    return lo, up


def lineage_rows(c, how=descend):
    rows = [how(c['parent'], c['vd'], c['val'], i, c['root_l'], c['root_u']) for i in c['ids']]
    return np.array([r[0] for r in rows]).reshape(len(c['ids']), c['n']), np.array([r[1] for r in rows]).reshape(len(c['ids']), c['n'])


def bounds_restated(c, how=descend):
    """out_l, out_u, out_v of treerec_bounds from sentinel-filled outputs."""
    k = len(c['ids'])
    l, u = lineage_rows(c, how)
    v = filled((k, c['nv']), np.int8)
    if c['root_v'] is not None:
        v[:] = c['root_v']
    return l, u, v


def seed_restated(c, how=descend):
    """the pool of restart_seed from a sentinel-filled pool of c['capacity'] rows."""
    cap = c['capacity']
    pl, pu, pv = filled((cap, c['n']), np.float64), filled((cap, c['n']), np.float64), filled((cap, c['nv']), np.int8)
    l, u = lineage_rows(c, how)
    for k, s in enumerate(c['slots']):
        if 0 <= s < cap:
            pl[s], pu[s] = l[k], u[k]
            pv[s] = c['root_v'] if c['root_v'] is not None else 0
    return pl, pu, pv


def _lineage_finish(c, rng, root_v=True, bad_slot=False):
    n, k = c['n'], len(c['ids'])
    c['ids'] = np.asarray(c['ids'], np.int64)
    c['parent'], c['vd'], c['val'] = np.asarray(c['parent'], np.int32), np.asarray(c['vd'], np.int32), np.asarray(c['val'], np.float64)
    c.setdefault('nv', n + 3)
    c['root_l'], c['root_u'] = rows_of(rng, 1, n)[0], rows_of(rng, 1, n)[0]
    c['root_v'] = rng.integers(-3, 6, c['nv']).astype(np.int8) if root_v else None
    c['capacity'] = k + 3
    c['slots'] = scattered_slots(rng, k, k + 3)
    if bad_slot:   # two seeds outside the pool: nothing of them is written
        c['slots'][k // 2], c['slots'][-1] = -1, c['capacity']
    return c


def _random_tree(rng, n, nodes, cols):
    parent, vd, val = [-1], [-2], [0.0]
    for i in range(1, nodes):
        parent.append(int(rng.integers(max(0, i - 6), i)))
        vd.append(2 * int(rng.choice(cols)) + int(rng.integers(0, 2)))
        val.append(float(rng.choice(BRANCH_VALUES)) if i % 3 else float(rng.normal() * 9.0))
    return parent, vd, val


def _lineage_case(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name.startswith('lineage-tree-n'):
        n = int(name.split('-n')[1])
        cols = sorted({j for j in (0, 1, 3, 254, 255, 256, 257, 259, 510, 511, 512, n - 1) if 0 <= j < n})
        parent, vd, val = _random_tree(rng, n, 40, cols)
        ids = list(rng.permutation(40)) + [17, 0]           # out of order, one id twice, the root twice
        return _lineage_finish(dict(n=n, nv=(n + 3 if n != 1024 else 2047), parent=parent, vd=vd, val=val, ids=ids), rng)
    if name == 'lineage-chain-3000':
        n, depth = 257, 3000
        cols = (0, 256, 1, 255, 128)                       # 0 and 256 belong to one thread
        parent = [-1] + list(range(depth))
        vd = [-2] + [2 * cols[(i // 3) % 5] + (i % 2) for i in range(1, depth + 1)]
        val = [0.0] + [float((i * 37) % 101) - 50.25 for i in range(1, depth + 1)]
        return _lineage_finish(dict(n=n, parent=parent, vd=vd, val=val, ids=[depth, 1, 2, depth - 1, 1500]), rng)
    if name == 'lineage-columns-n1024':
        n = 1024
        seq = [(255, 0), (256, 1), (257, 0), (511, 1), (1023, 0), (3, 1), (259, 1), (3, 0), (259, 0), (1023, 1), (767, 0), (255, 1)]
        parent = [-1] + list(range(len(seq)))
        vd = [-2] + [2 * j + d for j, d in seq]
        val = [0.0] + [BRANCH_VALUES[i % 6] + i for i in range(len(seq))]
        return _lineage_finish(dict(n=n, nv=2047, parent=parent, vd=vd, val=val, ids=[len(seq), 7, 5, 0, 1, 2]), rng)
    if name == 'lineage-same-column':
        n = 300
        #  column 260: left, right, left again;  column 4 (same thread as 260): right three times in a row
        seq = [(260, 0, 9.5), (260, 1, 2.5), (260, 0, 6.5), (4, 1, 1.5), (4, 1, 3.5), (4, 1, 2.5), (260, 0, 7.5)]
        parent = [-1] + list(range(len(seq)))
        vd = [-2] + [2 * j + d for j, d, _ in seq]
        val = [0.0] + [v for _, _, v in seq]
        return _lineage_finish(dict(n=n, parent=parent, vd=vd, val=val, ids=list(range(len(seq), -1, -1))), rng)
    if name == 'lineage-malformed':
        n = 258
        #  id:      0    1       2       3        4             5            6        7 (parent = itself)  8 (parent above)
        parent = [-1, 0, 1, 2, 3, 4, 5, 7, 9, 6]
        vd = [-2, 2 * 257, 2 * n, 2 * n + 1, -2, -(1 << 20) + 1, 2 * 1 + 1, 2 * 5, 2 * 6 + 1, 2 * 256]
        val = [0.0, 4.5, 1.5, 2.5, 3.5, 5.5, -0.5, 8.5, 9.5, 7.5]
        ids = [6, 7, 8, 9, 10, 1 << 40, 3, 4, 5]             # 10 and 2^40: outside the mirror
        return _lineage_finish(dict(n=n, parent=parent, vd=vd, val=val, ids=ids), rng, bad_slot=True)
    if name == 'lineage-no-root-codes':
        n = 65
        parent, vd, val = _random_tree(rng, n, 12, (0, 1, 64))
        return _lineage_finish(dict(n=n, parent=parent, vd=vd, val=val, ids=[11, 0, 5]), rng, root_v=False)
    if name == 'lineage-depth-1-2':
        n = 2
        return _lineage_finish(dict(n=n, parent=[-1, 0, 0, 1, 2], vd=[-2, 0, 1, 3, 2], val=[0.0, 2.5, 2.5, -0.5, 3.0],
                                    ids=[0, 1, 2, 3, 4]), rng)
    if name == 'lineage-two-chunks':                          # more ids than one launch of the engine takes (2^14)
        ids = [(7 * k) % 9 for k in range(LINEAGE_CHUNK + 5)]   # (7 and 8: outside the mirror)
        return _lineage_finish(dict(n=1, nv=2, parent=[-1, 0, 0, 1, 2, 3, 5], vd=[-2, 0, 1, 1, 0, 0, 1],
                                    val=[0.0, 7.5, 2.5, 3.5, 5.5, 6.5, 4.5], ids=ids), rng)
    if name == 'lineage-empty-mirror':
        return _lineage_finish(dict(n=1, parent=[], vd=[], val=[], ids=[0, 5]), rng)
    raise KeyError(name)


LINEAGE_CASES = ['lineage-tree-n%d' % n for n in WIDTHS_256] + [
    'lineage-chain-3000', 'lineage-columns-n1024', 'lineage-same-column', 'lineage-malformed', 'lineage-no-root-codes',
    'lineage-depth-1-2', 'lineage-empty-mirror', 'lineage-two-chunks']


# ---- cut migration -------------------------------------------------------------------------------------------------------
CUT_KC = (1, 63, 64)
CUT_COUNTS = (1, 3, 4, 5)


def cut_lists_restated(c):
    out = c['lists'].copy()
    for k, s in enumerate(c['slot']):
        nc = int(c['pool_ncut'][s])
        out[k, 0] = nc
        out[k, 1:] = 0
        out[k, 1:1 + nc] = c['pool_ids'][s, :nc]
    return out


def _cut_lists_case(kc, count, seed):
    rng = np.random.default_rng(seed)
    rows = count + 3
    ncut = rng.integers(0, kc + 1, rows).astype(np.int32)
    slot = scattered_slots(rng, count, rows)
    for i, v in enumerate((kc, 0, 1)[:count]):
        ncut[slot[i]] = v
    return dict(kc=kc, slot=slot, pool_ncut=ncut, pool_ids=rng.integers(1, 1 << 20, (rows, kc)).astype(np.int32),
                lists=filled((count, 1 + kc), np.int32))


def cut_unpack_restated(c):
    ncut, ids, bad = c['pool_ncut'].copy(), c['pool_ids'].copy(), 0
    for k, s in enumerate(c['slot']):
        nc = int(c['lists'][k, 0])
        refs = c['lists'][k, 1:1 + max(nc, 0)]
        if 0 <= nc <= c['kc'] and np.all((refs >= 0) & (refs < c['ctab'])):
            ncut[s] = nc
            ids[s, :nc] = c['base'] + refs
        else:
            ncut[s], bad = 0, bad + 1
    return ncut, ids, bad


def _cut_unpack_case(kc, base, ctab, seed, count=9):
    """good records mixed with nc = -1, nc = kc + 1, a ref of -1 and a ref equal to ctab (ctab = 0: nc = 0 alone is good)"""
    rng = np.random.default_rng(seed)
    rows = count + 3
    lists = np.zeros((count, 1 + kc), np.int32)
    what = []
    for k in range(count):
        kind = ('good-full', 'nc=-1', 'good-empty', 'nc=kc+1', 'ref=-1', 'good-one', 'ref=ctab', 'good', 'good-full')[k % 9]
        if ctab == 0 and kind.startswith('good'):
            kind = 'good-empty'
        nc = {'good-full': kc, 'good-empty': 0, 'good-one': 1, 'nc=-1': -1, 'nc=kc+1': kc + 1}.get(kind, int(rng.integers(1, kc + 1)))
        lists[k, 0] = nc
        lists[k, 1:] = rng.integers(0, max(ctab, 1), kc)
        if kind == 'ref=-1':
            lists[k, nc] = -1                                     # the last entry of the list
        if kind == 'ref=ctab':
            lists[k, 1] = ctab
        if 0 <= nc < kc:
            lists[k, 1 + nc:] = -5                                # past the list: never looked at
        what.append(kind)
    return dict(kc=kc, base=base, ctab=ctab, slot=scattered_slots(rng, count, rows), lists=lists, what=what,
                pool_ncut=filled(rows, np.int32), pool_ids=filled((rows, kc), np.int32))


def _cut_rows_case(n, count, base, seed):
    """gather: store rows src -> table; scatter: table -> store rows base .. base + count."""
    rng = np.random.default_rng(seed)
    store_rows = base + count + 2
    c = dict(n=n, base=base, tab_pi=rows_of(rng, count, n), tab_pi0=rows_of(rng, 1, count)[0], store_rows=store_rows)
    if base == 0:
        c['store_pi'], c['store_pi0'] = rows_of(rng, store_rows, n), rows_of(rng, 1, store_rows)[0]
        c['src'] = scattered_slots(rng, count, store_rows)
        if count > 2:
            c['src'][1] = c['src'][0]                             # one store row into two table rows
    return c


# ---- spill ---------------------------------------------------------------------------------------------------------------
def encode(root_l, root_u, l, u, v, ncut=None, cut_ids=None, node_id=None):
    """The record layout of include/mipx_spill.h, written out in numpy: (offsets int64 count + 1, bytes uint8)."""
    offsets, out = [0], []
    rl, ru = root_l.view(np.uint64), root_u.view(np.uint64)
    for k in range(l.shape[0]):
        diff = (l[k].view(np.uint64) != rl) | (u[k].view(np.uint64) != ru)
        cols = np.nonzero(diff)[0].astype(np.int32)
        nc = int(ncut[k]) if cut_ids is not None else 0
        rec = np.array([k if node_id is None else node_id[k]], np.int64).tobytes() + np.array([cols.size, nc], np.int32).tobytes()
        rec += pad8(cols.tobytes()) + l[k, cols].tobytes() + u[k, cols].tobytes()
        nib = (v[k].astype(np.int16) & 0xF).astype(np.uint8)
        if nib.size % 2:
            nib = np.append(nib, np.uint8(0))
        rec += pad8((nib[0::2] | (nib[1::2] << 4)).astype(np.uint8).tobytes())
        if cut_ids is not None:
            rec += pad8(cut_ids[k, :nc].astype(np.int32).tobytes())
        out.append(rec)
        offsets.append(offsets[-1] + len(rec))
    return np.array(offsets, np.int64), np.frombuffer(b''.join(out), np.uint8)


def decode(root_l, root_u, offsets, records, slot, l, u, v, ncut=None, ids=None):
    """spill_unpack: record r into row slot[r] (row r without a slot list) of copies of the pool's arrays."""
    l, u, v = l.copy(), u.copy(), v.copy()
    ncut, ids = (None, None) if ids is None else (ncut.copy(), ids.copy())
    nv, buf = v.shape[1], np.ascontiguousarray(records).tobytes()
    for r in range(len(offsets) - 1):
        row = r if slot is None else int(slot[r])
        p = int(offsets[r])
        nd, nc = np.frombuffer(buf, np.int32, 2, p + 8)
        cols = np.frombuffer(buf, np.int32, nd, p + 16)
        o_l = p + 16 + (4 * nd + 7) // 8 * 8
        l[row], u[row] = root_l, root_u
        l[row, cols] = np.frombuffer(buf, np.float64, nd, o_l)
        u[row, cols] = np.frombuffer(buf, np.float64, nd, o_l + 8 * nd)
        o_v = o_l + 16 * nd
        code = np.frombuffer(buf, np.uint8, (nv + 1) // 2, o_v)
        nib = np.stack([code & 0xF, code >> 4], 1).reshape(-1)[:nv].astype(np.int8)
        v[row] = np.where(nib >= 8, nib - 16, nib)
        if ids is not None:
            ncut[row] = nc
            ids[row, :nc] = np.frombuffer(buf, np.int32, nc, o_v + ((nv + 1) // 2 + 7) // 8 * 8)
    return (l, u, v) if ids is None else (l, u, v, ncut, ids)


def random_rows(rng, count, n, nv):
    specials = np.array([INF, -INF, 0.0, -0.0, 1.0, -1.0, 2.5, 1e300])
    root_l = rng.choice(specials, n)
    root_u = rng.choice(specials, n)
    l = np.tile(root_l, (count, 1))
    u = np.tile(root_u, (count, 1))
    for k in range(count):
        if k % 4 == 0:
            continue                       # no diff at all
        nd = n if k % 4 == 1 else int(rng.integers(1, n + 1))
        cols = rng.choice(n, nd, replace=False)
        l[k, cols] = rng.choice(np.concatenate([specials, rng.normal(size=4)]), nd)
        u[k, cols[: nd // 2]] = rng.choice(specials, nd // 2)
        if k % 4 == 2:                     # the sign of a zero alone is a difference
            z = np.flatnonzero(root_l == 0.0)
            l[k, z] = -root_l[z] if z.size else l[k, z]
    v = rng.integers(0, 6, (count, nv)).astype(np.int8)
    v.flat[:6] = np.arange(6)   # every code at least once
    return root_l, root_u, l, u, v


def _spill_case(n, nv, count, form, seed):
    """form: 'plain' (row r, id r), 'cut' (kc = 5, row r), 'slots' (a slot list into a larger pool, header ids given),
    'slots-cut' (both)."""
    rng = np.random.default_rng(seed)
    cut, slots = 'cut' in form, 'slots' in form
    kc = 5 if cut else 0
    rows = count + 7 if slots else count
    root_l, root_u, l, u, v = random_rows(rng, rows, n, nv)
    if nv >= 8:
        v[:, -3:] = (-1, -8, 7)            # two's complement in 4 bits: the sign comes back
    c = dict(n=n, nv=nv, kc=kc, count=count, form=form, root_l=root_l, root_u=root_u, l=l, u=u, v=v, ncut=None, ids=None,
             slot=None, node_id=None)
    if cut:
        c['ncut'] = rng.integers(0, kc + 1, rows).astype(np.int32)
        c['ncut'][:2] = (0, kc)[:rows]
        c['ids'] = rng.integers(0, 1 << 20, (rows, kc)).astype(np.int32)
    if slots:
        c['slot'] = scattered_slots(rng, count, rows)
        c['node_id'] = (rng.integers(0, 1 << 40, count) + (np.arange(count) << 41)).astype(np.int64)
    sel = np.arange(count) if not slots else c['slot']
    c['offsets'], c['records'] = encode(root_l, root_u, l[sel], u[sel], v[sel], c['ncut'][sel] if cut else None,
                                        c['ids'][sel] if cut else None, c['node_id'])
    return c


SPILL_SMALL = [(n, nv, count) for n, nv in zip(WIDTHS_64, (2, 65, 96, 67, 200, 2047)) for count in CUT_COUNTS]
SPILL_LARGE = [(3, 5, count) for count in (1023, 1024, 1025, 2049, 4100)]
SPILL_FORMS = ('plain', 'cut', 'slots', 'slots-cut')
SPILL_CASES = ['spill-%s-n%d-nv%d-count%d' % (f, n, nv, k) for f in SPILL_FORMS for n, nv, k in SPILL_SMALL + SPILL_LARGE
               if k >= 1023 or f in ('plain', 'slots-cut') or n in (65, 1024)]


def gather_rows_restated(c):
    l, u, v = c['l'].copy(), c['u'].copy(), c['v'].copy()
    for k, s in enumerate(c['slot']):
        if s >= 0:
            l[k], u[k], v[k] = c['src_l'][s], c['src_u'][s], c['src_v'][s]
    return l, u, v


def _gather_rows_case(n, nv, seed):
    rng = np.random.default_rng(seed)
    count, rows = 7, 6
    slot = np.array([5, -1, 0, 3, -2 - 4, 0, 2], np.int32)       # negative: on the host, left alone; row 0 twice
    return dict(n=n, nv=nv, slot=slot, src_l=rows_of(rng, rows, n), src_u=rows_of(rng, rows, n),
                src_v=rng.integers(-3, 6, (rows, nv)).astype(np.int8), l=filled((count, n), np.float64),
                u=filled((count, n), np.float64), v=filled((count, nv), np.int8))


GATHER_ROWS_CASES = ['gather-rows-n%d-nv%d' % s for s in MESSAGE_SHAPES]


# ---- the cases, by name, built once per process ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(name):
    seed = sum(map(ord, name))
    if name in CHILDREN_PLAIN:
        return _children_case(*CHILDREN_PLAIN[name], seed=seed)
    if name in CHILDREN_CUT:
        return _children_case(seed=seed, **CHILDREN_CUT[name])
    if name.startswith('message-'):
        n, nvs = (int(t[1:].lstrip('vs')) for t in name.split('-')[1:])
        return _message_case(n, nvs, 5, seed)
    if name.startswith('gather-rows-'):
        n, nv = (int(t.lstrip('nv')) for t in name.split('-')[2:])
        return _gather_rows_case(n, nv, seed)
    if name.startswith('gather-'):
        n, m, pool = (int(t.lstrip('nmpol')) for t in name.split('-')[1:])
        rng = np.random.default_rng(seed)
        rows, count = 8, 5
        return dict(n=n, m=m, nvs_pool=pool, slot=scattered_slots(rng, count, rows), pool_l=rows_of(rng, rows, n),
                    pool_u=rows_of(rng, rows, n), pool_v=rng.integers(-3, 6, (rows, pool)).astype(np.int8),
                    l=filled((count, n), np.float64), u=filled((count, n), np.float64), v=filled((count, n + m), np.int8))
    if name.startswith('lineage-'):
        return _lineage_case(name)
    if name.startswith('spill-'):
        form, n, nv, count = re.fullmatch(r'spill-([a-z-]+)-n(\d+)-nv(\d+)-count(\d+)', name).groups()
        return _spill_case(int(n), int(nv), int(count), form, seed)
    raise KeyError(name)
