"""The kernels that move node rows on synthetic pools (include/mipx_noderows.h), bit for bit against the plain
restatements of tests/support/node_rows_reference.py: make_children, pack_nodes / unpack_nodes / gather_plain_nodes,
treerec_bounds / restart_seed, the four cutmig_* kernels and the five spill_* kernels, at every width at which their
loops take another trip, with sentinel-filled (0x5a) outputs so that a byte written past a row shows.  No tolerance
appears here: doubles are compared as bytes."""
import numpy as np
import pytest

from simple_mip_solver_amd import _ffi
from tests.support import node_rows_reference as ref

pytestmark = pytest.mark.gpu


def check(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        g, w = got.reshape(-1).view(np.uint8), want.reshape(-1).view(np.uint8)
        at = int(np.flatnonzero(g != w)[0]) // got.itemsize
        idx = np.unravel_index(at, got.shape)
        raise AssertionError(f'{what}: first difference at {idx}: got {got[idx]!r}, want {want[idx]!r}')


def refused(ctx, call, inout, match):
    """`call` raises with `match` in the message and leaves every in-and-out array as it was."""
    before = [a.copy() for a in inout]
    with pytest.raises(_ffi.MipxError, match=match):
        call()
    for a, b in zip(inout, before):
        assert a.tobytes() == b.tobytes(), match


def raw_refusals(ctx, entry, args, inout, bad):
    """The C entry `entry` on `args` (a dict in the order of its parameters behind ctx: arrays, scalars or None), once per
    (overrides, match) of `bad`: MIPX_EINVAL, `match` in the message, every in-and-out array (the keys `inout`) as it
    was.  Then the call as given, which must be accepted."""
    L, h = _ffi.lib(), ctx._h
    before = {k: args[k].copy() for k in inout}

    def call(**kw):
        a = dict(args, **kw)
        vals = [v if v is None or np.isscalar(v) else np.ascontiguousarray(v) for v in a.values()]   # (alive over the call)
        return getattr(L, entry)(h, *(v if v is None or np.isscalar(v) else _ffi._ptr(v) for v in vals))
    for kw, match in bad:
        assert set(kw) <= set(args), kw
        assert call(**kw) == -1, (entry, kw)                              # MIPX_EINVAL
        assert match in L.mipx_last_error(h).decode(), (entry, kw, L.mipx_last_error(h).decode())
        assert all(args[k].tobytes() == before[k].tobytes() for k in inout), (entry, kw)
    assert call() == 0, (entry, L.mipx_last_error(h).decode())


def with_entry(a, key, at, value):
    b = np.array(a[key], copy=True)
    b[at] = value
    return {key: b}


# ---- children ------------------------------------------------------------------------------------------------------------
CHILD_IN = ('src_l', 'src_u', 'x', 'vstat', 'parent_slot', 'parent_pos', 'var', 'child_slot')


def run_children(ctx, c, pairs=None, out=None):
    out = out or {k: c[k].copy() for k in ('dst_l', 'dst_u', 'dst_v', 'dst_ncut', 'dst_ids') if c[k] is not None}
    a = {k: c[k] for k in CHILD_IN}
    if pairs is not None:
        a.update(parent_slot=c['parent_slot'][pairs], parent_pos=c['parent_pos'][pairs], var=c['var'][pairs],
                 child_slot=c['child_slot'].reshape(-1, 2)[pairs].reshape(-1))
    _ffi.noderows_children(ctx, c['n'], c['m'], *(a[k] for k in CHILD_IN), out['dst_l'], out['dst_u'], out['dst_v'],
                           mstride=c['mstride'], kc=c['kc'], src_ncut=c['src_ncut'], src_ids=c['src_ids'],
                           dst_ncut=out.get('dst_ncut'), dst_ids=out.get('dst_ids'))
    return out


@pytest.mark.parametrize('name', ref.CHILDREN_CASES)
def test_children_are_the_parent_row_with_one_bound_moved(name, gpu_ctx):
    c = ref.case(name)
    got, want = run_children(gpu_ctx, c), ref.children_restated(c)
    for k in want:
        check(got[k], want[k], f'{name} {k}')


@pytest.mark.parametrize('name', ['children-n257-m8', 'children-cut-kc64-loose'])
def test_children_one_call_or_one_call_per_pair(name, gpu_ctx):
    c = ref.case(name)
    whole, out = run_children(gpu_ctx, c), None
    for p in range(len(c['var'])):
        out = run_children(gpu_ctx, c, pairs=[p], out=out)
    for k in whole:
        check(out[k], whole[k], f'{name} {k}')


def test_children_refusals(gpu_ctx):
    c = ref.case('children-cut-kc64-loose')
    out = {k: c[k].copy() for k in ('dst_l', 'dst_u', 'dst_v', 'dst_ncut', 'dst_ids')}
    L, h, p = _ffi.lib(), gpu_ctx._h, _ffi._ptr
    dst_rows, pos0 = len(out['dst_l']), int(c['parent_pos'][0])

    def call(**kw):
        a = dict(c, count=len(c['var']), src_rows=5, batch_rows=6, dst_rows=dst_rows, **out)
        a.update(kw)
        keep = [np.ascontiguousarray(a[k]) if a[k] is not None and not np.isscalar(a[k]) else a[k] for k in a]   # (alive over the call)
        a = dict(zip(a, keep))
        q = lambda k: p(a[k])   # noqa: E731
        return L.mipx_noderows_children(h, a['n'], a['m'], a['mstride'], a['kc'], a['count'], a['src_rows'], q('src_l'), q('src_u'),
                                        a['batch_rows'], q('x'), q('vstat'), q('src_ncut'), q('src_ids'), q('parent_slot'),
                                        q('parent_pos'), q('var'), q('child_slot'), a['dst_rows'], q('dst_l'), q('dst_u'), q('dst_v'),
                                        q('dst_ncut'), q('dst_ids'))

    def one(key, at, value):
        a = c[key].copy()
        a[at] = value
        return {key: a}
    twice = c['child_slot'].copy()
    twice[3] = twice[0]
    bad = [(one('parent_slot', 1, 5), 'parent_slot outside'), (one('parent_slot', 0, -1), 'parent_slot outside'),
           (one('parent_pos', 2, 6), 'parent_pos outside'), (one('parent_pos', 2, -1), 'parent_pos outside'),
           (one('var', 0, c['n']), 'var outside'), (one('var', 1, -1), 'var outside'),
           (one('child_slot', 5, dst_rows), 'child_slot outside'), (one('child_slot', 0, -1), 'child_slot outside'),
           (dict(child_slot=twice), 'two equal child slots'), (dict(kc=65), 'kc outside'), (dict(kc=-1), 'kc outside'),
           (one('src_ncut', pos0, 65), 'src_ncut outside'), (one('src_ncut', pos0, -1), 'src_ncut outside'),
           (dict(mstride=c['m'] + 63), 'm + kc > mstride'), (dict(src_l=None), 'null'), (dict(x=None), 'null'),
           (dict(src_ncut=None), 'null'), (dict(dst_ids=None), 'null'), (dict(var=None), 'null'),
           (dict(mstride=0), 'plain mode'), (dict(mstride=0, kc=0), 'plain mode'),
           (dict(n=0), '< 1'), (dict(m=0), '< 1'), (dict(src_rows=0), '< 1'), (dict(batch_rows=0), '< 1'), (dict(dst_rows=0), '< 1'),
           (dict(count=-1), 'count < 0')]
    for kw, match in bad:
        assert call(**kw) == -1, match                                   # MIPX_EINVAL
        assert match in L.mipx_last_error(h).decode(), (match, L.mipx_last_error(h).decode())
        assert all(out[k].tobytes() == c[k].tobytes() for k in out), match
    assert call() == 0
    for k, v in ref.children_restated(c).items():
        check(out[k], v, k)


# ---- message -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ref.MESSAGE_CASES)
def test_message_rows_are_the_documented_bytes_and_unpack_inverts_them(name, gpu_ctx):
    c = ref.case(name)
    n, nvs, slot, other = c['n'], c['nvs'], c['slot'], c['other']
    rb = ref.rowbytes(n, nvs)
    msg = ref.filled((len(slot), rb), np.uint8)
    _ffi.noderows_pack(gpu_ctx, n, nvs, slot, c['pool_l'], c['pool_u'], c['pool_v'], msg)
    want = ref.message_packed(n, nvs, slot, c['pool_l'], c['pool_u'], c['pool_v'], ref.filled((len(slot), rb), np.uint8))
    check(msg, want, f'{name} message')
    assert np.all(msg[:, 16 * n + nvs:] == ref.FILL)                    # the pad bytes are what they were
    rows = len(c['pool_l']) + 2
    pool = [ref.filled((rows, n), np.float64), ref.filled((rows, n), np.float64), ref.filled((rows, nvs), np.int8)]
    wantp = ref.message_unpacked(n, nvs, other, msg, *pool)
    _ffi.noderows_unpack(gpu_ctx, n, nvs, other, msg, *pool)
    for g, w, k in zip(pool, wantp, 'luv'):
        check(g, w, f'{name} pool {k}')
        check(g[other], c['pool_' + k][slot], f'{name} rows {k}')
    again = ref.filled((len(slot), rb), np.uint8)
    _ffi.noderows_pack(gpu_ctx, n, nvs, other, *pool, again)
    check(again, msg, f'{name} packed again')


def test_message_one_call_or_one_call_per_row(gpu_ctx):
    c = ref.case('message-n257-nvs258')
    n, nvs, slot = c['n'], c['nvs'], c['slot']
    rb = ref.rowbytes(n, nvs)
    whole = ref.filled((len(slot), rb), np.uint8)
    _ffi.noderows_pack(gpu_ctx, n, nvs, slot, c['pool_l'], c['pool_u'], c['pool_v'], whole)
    pool = [ref.filled(c['pool_' + k].shape, c['pool_' + k].dtype) for k in 'luv']
    for k, s in enumerate(slot):
        one = ref.filled((1, rb), np.uint8)
        _ffi.noderows_pack(gpu_ctx, n, nvs, [s], c['pool_l'], c['pool_u'], c['pool_v'], one)
        check(one[0], whole[k], f'row {k}')
        _ffi.noderows_unpack(gpu_ctx, n, nvs, [s], one, *pool)
    together = [ref.filled(c['pool_' + k].shape, c['pool_' + k].dtype) for k in 'luv']
    _ffi.noderows_unpack(gpu_ctx, n, nvs, slot, whole, *together)
    for g, w, k in zip(pool, together, 'luv'):
        check(g, w, f'pool {k}')


def test_message_refusals(gpu_ctx):
    c = ref.case('message-n2-nvs7')
    n, nvs, slot = c['n'], c['nvs'], c['slot']
    rows = len(c['pool_l'])
    msg = ref.filled((len(slot), ref.rowbytes(n, nvs)), np.uint8)
    pool = [c['pool_l'].copy(), c['pool_u'].copy(), c['pool_v'].copy()]
    for s, match in (([rows] + list(slot[1:]), 'slot outside'), ([-1] + list(slot[1:]), 'slot outside')):
        refused(gpu_ctx, lambda: _ffi.noderows_pack(gpu_ctx, n, nvs, s, *pool, msg), [msg], match)
        refused(gpu_ctx, lambda: _ffi.noderows_unpack(gpu_ctx, n, nvs, s, msg, *pool), pool, match)
    refused(gpu_ctx, lambda: _ffi.noderows_unpack(gpu_ctx, n, nvs, [1, 2, 1, 0, 3], msg, *pool), pool, 'two equal slots')
    L, h, p = _ffi.lib(), gpu_ctx._h, _ffi._ptr
    sl = np.asarray(slot, np.int32)
    for args in ((0, nvs, 5, p(sl), rows), (n, 0, 5, p(sl), rows), (n, nvs, -1, p(sl), rows), (n, nvs, 5, p(sl), 0), (n, nvs, 5, None, rows)):
        assert L.mipx_noderows_pack(h, *args, p(pool[0]), p(pool[1]), p(pool[2]), p(msg)) == -1
        assert L.mipx_noderows_unpack(h, *args[:4], p(msg), args[4], p(pool[0]), p(pool[1]), p(pool[2])) == -1
    assert L.mipx_noderows_pack(h, n, nvs, 5, p(sl), rows, None, p(pool[1]), p(pool[2]), p(msg)) == -1
    assert L.mipx_noderows_unpack(h, n, nvs, 5, p(sl), None, rows, p(pool[0]), p(pool[1]), p(pool[2])) == -1
    assert np.all(msg == ref.FILL) and all(a.tobytes() == c['pool_' + k].tobytes() for a, k in zip(pool, 'luv'))


@pytest.mark.parametrize('name', ref.GATHER_CASES)
def test_gather_plain_takes_the_shared_codes_of_a_wider_pool(name, gpu_ctx):
    c = ref.case(name)
    got = [c[k].copy() for k in 'luv']
    _ffi.noderows_gather_plain(gpu_ctx, c['n'], c['m'], c['nvs_pool'], c['slot'], c['pool_l'], c['pool_u'], c['pool_v'], *got)
    for g, w, k in zip(got, ref.gather_plain_restated(c), 'luv'):
        check(g, w, f'{name} {k}')


def test_gather_plain_refusals(gpu_ctx):
    c = ref.case('gather-n2-m3-pool6')
    got = [c[k].copy() for k in 'luv']

    def call(n=c['n'], m=c['m'], pool=c['nvs_pool'], slot=c['slot'], pool_l=c['pool_l']):
        _ffi.noderows_gather_plain(gpu_ctx, n, m, pool, slot, pool_l, c['pool_u'], c['pool_v'], *got)
    refused(gpu_ctx, lambda: call(pool=4), got, 'nvs_pool < n')
    refused(gpu_ctx, lambda: call(slot=[0, 8, 1, 2, 3]), got, 'slot outside')
    refused(gpu_ctx, lambda: call(slot=[0, -1, 1, 2, 3]), got, 'slot outside')
    refused(gpu_ctx, lambda: call(m=0, pool=12), got, '< 1')
    L, h, p = _ffi.lib(), gpu_ctx._h, _ffi._ptr
    sl = np.asarray(c['slot'], np.int32)
    arrs = [p(c['pool_l']), p(c['pool_u']), p(c['pool_v'])] + [p(a) for a in got]
    assert L.mipx_noderows_gather_plain(h, 0, 3, 6, 5, p(sl), 8, *arrs) == -1
    assert L.mipx_noderows_gather_plain(h, 2, 3, 6, -1, p(sl), 8, *arrs) == -1
    assert L.mipx_noderows_gather_plain(h, 2, 3, 6, 5, p(sl), 0, *arrs) == -1
    assert L.mipx_noderows_gather_plain(h, 2, 3, 6, 5, p(sl), 8, None, *arrs[1:]) == -1
    assert L.mipx_noderows_gather_plain(h, 2, 3, 6, 5, p(sl), 8, *arrs[:5], None) == -1
    assert all(np.all(a.view(np.uint8) == ref.FILL) for a in got)


# ---- lineage -------------------------------------------------------------------------------------------------------------
def run_bounds(ctx, c, ids=None, out=None):
    ids = c['ids'] if ids is None else ids
    out = out or [ref.filled((len(ids), c['n']), np.float64), ref.filled((len(ids), c['n']), np.float64),
                  ref.filled((len(ids), c['nv']), np.int8)]
    _ffi.noderows_lineage_bounds(ctx, c['n'], c['nv'], c['parent'], c['vd'], c['val'], ids, c['root_l'], c['root_u'], c['root_v'], *out)
    return out


def run_seed(ctx, c, sel=None, pool=None):
    cap = c['capacity']
    pool = pool or [ref.filled((cap, c['n']), np.float64), ref.filled((cap, c['n']), np.float64), ref.filled((cap, c['nv']), np.int8)]
    sel = slice(None) if sel is None else sel
    _ffi.noderows_lineage_seed(ctx, c['n'], c['nv'], c['parent'], c['vd'], c['val'], c['ids'][sel], c['slots'][sel], c['root_l'],
                               c['root_u'], c['root_v'], *pool)
    return pool


@pytest.mark.parametrize('name', ref.LINEAGE_CASES)
def test_lineage_rows_are_the_branchings_applied_root_down(name, gpu_ctx):
    c = ref.case(name)
    got, want = run_bounds(gpu_ctx, c), ref.bounds_restated(c)
    for g, w, k in zip(got, want, 'luv'):
        check(g, w, f'{name} bounds {k}')
    if c['root_v'] is None:
        assert np.all(got[2] == ref.FILL)                               # out_v is left alone
    pool, wantp = run_seed(gpu_ctx, c), ref.seed_restated(c)
    for g, w, k in zip(pool, wantp, 'luv'):
        check(g, w, f'{name} seed {k}')
    inside = np.flatnonzero((c['slots'] >= 0) & (c['slots'] < c['capacity']))
    assert len(inside) >= len(c['ids']) - 2
    for g, p, k in zip(got[:2], pool[:2], 'lu'):                        # for every id the two kernels write the same bits
        check(p[c['slots'][inside]], g[inside], f'{name} seed against bounds {k}')
    if c['root_v'] is None:
        assert not pool[2][c['slots'][inside]].any()                    # a cold start: zero codes


@pytest.mark.parametrize('name', ['lineage-tree-n513', 'lineage-malformed', 'lineage-same-column'])
def test_lineage_one_call_or_one_call_per_id(name, gpu_ctx):
    c = ref.case(name)
    whole, wholep, pool = run_bounds(gpu_ctx, c), run_seed(gpu_ctx, c), None
    for k in range(len(c['ids'])):
        one = run_bounds(gpu_ctx, c, ids=c['ids'][k:k + 1])
        for g, w, key in zip(one, whole, 'luv'):
            check(g[0], w[k], f'{name} id {k} {key}')
        pool = run_seed(gpu_ctx, c, sel=slice(k, k + 1), pool=pool)
    for g, w, key in zip(pool, wholep, 'luv'):
        check(g, w, f'{name} seed {key}')


def test_lineage_refusals(gpu_ctx):
    c = ref.case('lineage-depth-1-2')
    out = [ref.filled((5, 2), np.float64), ref.filled((5, 2), np.float64), ref.filled((5, c['nv']), np.int8)]
    pool = [ref.filled((c['capacity'], 2), np.float64), ref.filled((c['capacity'], 2), np.float64), ref.filled((c['capacity'], c['nv']), np.int8)]
    L, h, p = _ffi.lib(), gpu_ctx._h, _ffi._ptr
    par, vd, val, ids, sl = c['parent'], c['vd'], c['val'], c['ids'], c['slots']
    rl, ru, rv = c['root_l'], c['root_u'], c['root_v']
    neg = ids.copy()
    neg[2] = -1
    same = sl.copy()
    same[3] = same[1]

    def bounds(n=2, nv=c['nv'], N=5, par=p(par), count=5, ids=p(ids), rl=p(rl), out_l=p(out[0]), out_v=p(out[2])):
        return L.mipx_noderows_lineage_bounds(h, n, nv, N, par, p(vd), p(val), count, ids, rl, p(ru), p(rv), out_l, p(out[1]), out_v)

    def seed(n=2, nv=c['nv'], N=5, par=p(par), count=5, ids=p(ids), sl=p(sl), cap=c['capacity'], rl=p(rl), pool_l=p(pool[0])):
        return L.mipx_noderows_lineage_seed(h, n, nv, N, par, p(vd), p(val), count, ids, sl, cap, rl, p(ru), p(rv), pool_l, p(pool[1]), p(pool[2]))
    for f in (bounds, seed):
        for kw in (dict(n=0), dict(n=1025), dict(nv=0), dict(N=-1), dict(count=-1), dict(ids=p(neg)), dict(par=None), dict(ids=None), dict(rl=None)):
            assert f(**kw) == -1, (f.__name__, list(kw))
    assert bounds(out_l=None) == -1 and bounds(out_v=None) == -1
    assert seed(pool_l=None) == -1 and seed(sl=None) == -1 and seed(cap=0) == -1 and seed(sl=p(same)) == -1
    assert 'two equal slots' in _ffi.lib().mipx_last_error(h).decode()
    assert all(np.all(a.view(np.uint8) == ref.FILL) for a in out + pool)
    assert bounds() == 0 and seed() == 0


# ---- cut migration -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('count', ref.CUT_COUNTS)
@pytest.mark.parametrize('kc', ref.CUT_KC)
def test_cut_lists_of_the_donor(kc, count, gpu_ctx):
    c = ref._cut_lists_case(kc, count, 100 * kc + count)
    got = c['lists'].copy()
    _ffi.noderows_cut_lists(gpu_ctx, kc, c['slot'], c['pool_ncut'], c['pool_ids'], got)
    check(got, ref.cut_lists_restated(c), f'kc {kc} count {count}')
    assert sorted(c['pool_ncut'][c['slot']][:3].tolist()) == sorted((kc, 0, 1)[:count])


@pytest.mark.parametrize('count', ref.CUT_COUNTS)
@pytest.mark.parametrize('n', ref.WIDTHS_64)
def test_cut_rows_gather_and_scatter(n, count, gpu_ctx):
    c = ref._cut_rows_case(n, count, 0, 10 * n + count)
    tab = [ref.filled((count, n), np.float64), ref.filled(count, np.float64)]
    _ffi.noderows_cut_gather(gpu_ctx, n, c['src'], c['store_pi'], c['store_pi0'], *tab)
    check(tab[0], c['store_pi'][c['src']], f'n {n} count {count} table')
    check(tab[1], c['store_pi0'][c['src']], f'n {n} count {count} table pi0')
    rows = count + 5
    for base in (0, 3):
        store = [ref.filled((rows, n), np.float64), ref.filled(rows, np.float64)]
        want = [a.copy() for a in store]
        want[0][base:base + count], want[1][base:base + count] = c['tab_pi'], c['tab_pi0']
        _ffi.noderows_cut_scatter(gpu_ctx, n, base, c['tab_pi'], c['tab_pi0'], *store)
        check(store[0], want[0], f'n {n} count {count} base {base} store')
        check(store[1], want[1], f'n {n} count {count} base {base} store pi0')


@pytest.mark.parametrize('n,count', [(1, 5), (2, 3)])
def test_cut_rows_scatter_at_a_far_base(n, count, gpu_ctx):
    base = 2 ** 20 - 2 ** 16
    c = ref._cut_rows_case(n, count, base, n)
    rows = c['store_rows']
    store = [ref.filled((rows, n), np.float64), ref.filled(rows, np.float64)]
    _ffi.noderows_cut_scatter(gpu_ctx, n, base, c['tab_pi'], c['tab_pi0'], *store)
    check(store[0][base:base + count], c['tab_pi'], 'rows')
    check(store[1][base:base + count], c['tab_pi0'], 'pi0')
    for a in store:
        rest = np.delete(a, np.s_[base:base + count], axis=0)
        assert np.all(rest.view(np.uint8) == ref.FILL)
    back = [ref.filled((count, n), np.float64), ref.filled(count, np.float64)]
    _ffi.noderows_cut_gather(gpu_ctx, n, np.arange(base, base + count)[::-1], *store, *back)
    check(back[0], c['tab_pi'][::-1], 'gathered back')
    check(back[1], c['tab_pi0'][::-1], 'gathered back pi0')


@pytest.mark.parametrize('base,ctab', [(0, 7), (2 ** 20 - 2 ** 16, 50), (5, 0)])
@pytest.mark.parametrize('kc', ref.CUT_KC)
def test_cut_lists_of_the_receiver_count_what_does_not_fit(kc, base, ctab, gpu_ctx):
    c = ref._cut_unpack_case(kc, base, ctab, 7 * kc + ctab)
    ncut, ids = c['pool_ncut'].copy(), c['pool_ids'].copy()
    bad = _ffi.noderows_cut_unpack_lists(gpu_ctx, kc, c['slot'], c['lists'], base, ctab, ncut, ids)
    want_ncut, want_ids, want_bad = ref.cut_unpack_restated(c)
    check(ncut, want_ncut, 'ncut')
    check(ids, want_ids, 'ids')
    assert bad == want_bad and bad == sum(not w.startswith('good') for w in c['what'])
    for k, w in enumerate(c['what']):
        if not w.startswith('good'):                                    # ncut = 0 and the ids untouched
            assert ncut[c['slot'][k]] == 0 and np.all(ids[c['slot'][k]].view(np.uint8) == ref.FILL), w


@pytest.mark.parametrize('count', [1, 3, 5])
def test_cut_lists_of_the_receiver_in_a_partial_block(count, gpu_ctx):
    c = ref._cut_unpack_case(63, 11, 9, count, count=count)
    ncut, ids = c['pool_ncut'].copy(), c['pool_ids'].copy()
    bad = _ffi.noderows_cut_unpack_lists(gpu_ctx, 63, c['slot'], c['lists'], 11, 9, ncut, ids)
    want_ncut, want_ids, want_bad = ref.cut_unpack_restated(c)
    check(ncut, want_ncut, 'ncut')
    check(ids, want_ids, 'ids')
    assert bad == want_bad


def test_cut_lists_refusals(gpu_ctx):
    c = ref._cut_lists_case(5, 4, 1)
    args = dict(kc=5, count=4, slot=c['slot'], pool_rows=7, pool_ncut=c['pool_ncut'], pool_ids=c['pool_ids'], lists=c['lists'].copy())
    raw_refusals(gpu_ctx, 'mipx_noderows_cut_lists', args, ['lists'], [
        (dict(kc=0), 'kc outside'), (dict(kc=65), 'kc outside'), (dict(pool_rows=0), 'pool_rows < 1'), (dict(count=-1), 'count < 0'),
        (with_entry(args, 'slot', 2, 7), 'slot outside'), (with_entry(args, 'slot', 1, -1), 'slot outside'),
        (dict(slot=None), 'null'), (dict(pool_ncut=None), 'null'), (dict(pool_ids=None), 'null'), (dict(lists=None), 'null')])
    check(args['lists'], ref.cut_lists_restated(c), 'lists')


def test_cut_gather_refusals(gpu_ctx):
    r = ref._cut_rows_case(3, 4, 0, 5)
    args = dict(n=3, count=4, src=r['src'], store_rows=6, store_pi=r['store_pi'], store_pi0=r['store_pi0'],
                tab_pi=ref.filled((4, 3), np.float64), tab_pi0=ref.filled(4, np.float64))
    raw_refusals(gpu_ctx, 'mipx_noderows_cut_gather', args, ['tab_pi', 'tab_pi0'], [
        (dict(n=0), 'n or store_rows < 1'), (dict(store_rows=0), 'n or store_rows < 1'), (dict(count=-1), 'count < 0'),
        (with_entry(args, 'src', 2, 6), 'src outside'), (with_entry(args, 'src', 1, -1), 'src outside'),
        (dict(src=None), 'null'), (dict(store_pi=None), 'null'), (dict(store_pi0=None), 'null'), (dict(tab_pi=None), 'null'),
        (dict(tab_pi0=None), 'null')])
    check(args['tab_pi'], r['store_pi'][r['src']], 'table')


def test_cut_scatter_refusals(gpu_ctx):
    r = ref._cut_rows_case(3, 4, 0, 5)
    args = dict(n=3, count=4, base=2, tab_pi=r['tab_pi'], tab_pi0=r['tab_pi0'], store_rows=6, store_pi=ref.filled((6, 3), np.float64),
                store_pi0=ref.filled(6, np.float64))
    raw_refusals(gpu_ctx, 'mipx_noderows_cut_scatter', args, ['store_pi', 'store_pi0'], [
        (dict(n=0), 'n or store_rows < 1'), (dict(store_rows=0), 'n or store_rows < 1'), (dict(count=-1), 'count or base < 0'),
        (dict(base=-1), 'count or base < 0'), (dict(base=3), 'base + count > store_rows'), (dict(store_rows=5), 'base + count > store_rows'),
        (dict(tab_pi=None), 'null'), (dict(tab_pi0=None), 'null'), (dict(store_pi=None), 'null'), (dict(store_pi0=None), 'null')])
    check(args['store_pi'][2:], r['tab_pi'], 'store')


def test_cut_unpack_lists_refusals(gpu_ctx):
    u = ref._cut_unpack_case(5, 3, 4, 2)
    args = dict(kc=5, count=9, slot=u['slot'], lists=u['lists'], base=3, ctab=4, pool_rows=12, pool_ncut=u['pool_ncut'].copy(),
                pool_ids=u['pool_ids'].copy(), bad=np.full(1, -1, np.int32))
    raw_refusals(gpu_ctx, 'mipx_noderows_cut_unpack_lists', args, ['pool_ncut', 'pool_ids', 'bad'], [
        (dict(kc=0), 'kc outside'), (dict(kc=65), 'kc outside'), (dict(pool_rows=0), 'pool_rows < 1'), (dict(count=-1), 'base or ctab < 0'),
        (dict(base=-1), 'base or ctab < 0'), (dict(ctab=-1), 'base or ctab < 0'), (dict(base=2 ** 31 - 4), 'INT32_MAX'),
        (with_entry(args, 'slot', 0, 12), 'slot outside'), (with_entry(args, 'slot', 3, -1), 'slot outside'),
        (with_entry(args, 'slot', 4, int(u['slot'][2])), 'two equal slots'),
        (dict(slot=None), 'null'), (dict(lists=None), 'null'), (dict(pool_ncut=None), 'null'), (dict(pool_ids=None), 'null'),
        (dict(bad=None), 'null')])
    want_ncut, want_ids, want_bad = ref.cut_unpack_restated(u)
    check(args['pool_ncut'], want_ncut, 'ncut')
    check(args['pool_ids'], want_ids, 'ids')
    assert args['bad'][0] == want_bad


# ---- spill ---------------------------------------------------------------------------------------------------------------
def spill_pool(c, sentinel):
    keys = ('l', 'u', 'v') + (('ncut', 'ids') if c['kc'] else ())
    return [ref.filled(c[k].shape, c[k].dtype) if sentinel else c[k] for k in keys]


@pytest.mark.parametrize('name', ref.SPILL_CASES)
def test_spill_records_offsets_and_their_way_back(name, gpu_ctx):
    c = ref.case(name)
    n, nv, kc, count = c['n'], c['nv'], c['kc'], c['count']
    total = int(c['offsets'][-1])
    off, rec = ref.filled(count + 1, np.int64), ref.filled(total + 64, np.uint8)
    used = _ffi.noderows_spill_pack(gpu_ctx, n, nv, kc, count, c['root_l'], c['root_u'], c['l'], c['u'], c['v'], c['ncut'], c['ids'],
                                    c['slot'], c['node_id'], off, rec)
    assert used == total
    check(off, c['offsets'], f'{name} offsets')
    check(rec[:total], c['records'], f'{name} records')
    assert np.all(rec[total:] == ref.FILL)
    pool = spill_pool(c, True)
    _ffi.noderows_spill_unpack(gpu_ctx, n, nv, kc, c['root_l'], c['root_u'], off, rec[:total], c['slot'], *pool)
    want = ref.decode(c['root_l'], c['root_u'], c['offsets'], c['records'], c['slot'], *spill_pool(c, True))
    sel = np.arange(count) if c['slot'] is None else c['slot']
    for g, w, k in zip(pool, want, ('l', 'u', 'v', 'ncut', 'ids')):
        check(g, w, f'{name} pool {k}')
        if k != 'ids':
            check(g[sel], c[k][sel], f'{name} rows {k}')


def test_spill_pack_reports_the_room_it_needs(gpu_ctx):
    c = ref.case('spill-slots-cut-n65-nv67-count5')
    off, rec = ref.filled(6, np.int64), ref.filled(64, np.uint8)
    used = np.zeros(1, np.int64)
    p = _ffi._ptr
    rc = _ffi.lib().mipx_noderows_spill_pack(gpu_ctx._h, 65, 67, 5, 5, p(c['root_l']), p(c['root_u']), len(c['l']), p(c['l']), p(c['u']),
                                             p(c['v']), p(c['ncut']), p(c['ids']), p(c['slot']), p(c['node_id']), p(off), p(rec), 64,
                                             p(used))
    assert rc == -5 and used[0] == c['offsets'][-1]                     # MIPX_ENOMEM
    check(off, c['offsets'], 'offsets')
    assert np.all(rec == ref.FILL)


SPILL_REFUSAL_CASE = 'spill-slots-cut-n65-nv67-count5'


def test_spill_pack_refusals(gpu_ctx):
    c = ref.case(SPILL_REFUSAL_CASE)
    rows, total = len(c['l']), int(c['offsets'][-1])
    args = dict(n=65, nv=67, kc=5, count=5, root_l=c['root_l'], root_u=c['root_u'], pool_rows=rows, l=c['l'], u=c['u'], v=c['v'],
                ncut=c['ncut'], ids=c['ids'], slot=c['slot'], node_id=c['node_id'], out_offsets=ref.filled(6, np.int64),
                out_bytes=ref.filled(total, np.uint8), cap=total, used=np.full(1, -1, np.int64))
    raw_refusals(gpu_ctx, 'mipx_noderows_spill_pack', args, ['out_offsets', 'out_bytes', 'used'], [
        (dict(n=0), 'n, nv or pool_rows < 1'), (dict(nv=0), 'n, nv or pool_rows < 1'), (dict(pool_rows=0), 'n, nv or pool_rows < 1'),
        (dict(count=-1), 'count or cap < 0'), (dict(cap=-1), 'count or cap < 0'), (dict(kc=65), 'kc outside'), (dict(kc=-1), 'kc outside'),
        (with_entry(args, 'slot', 0, rows), 'slot outside'), (with_entry(args, 'slot', 1, -1), 'slot outside'),
        (dict(slot=None, count=rows + 1), 'slot outside'),
        (with_entry(args, 'ncut', int(c['slot'][1]), 6), 'ncut outside'), (with_entry(args, 'ncut', int(c['slot'][4]), -1), 'ncut outside'),
        (dict(root_l=None), 'null'), (dict(root_u=None), 'null'), (dict(l=None), 'null'), (dict(u=None), 'null'), (dict(v=None), 'null'),
        (dict(ncut=None), 'null'), (dict(ids=None), 'null'), (dict(out_offsets=None), 'null'), (dict(out_bytes=None), 'null'),
        (dict(used=None), 'null')])
    check(args['out_offsets'], c['offsets'], 'offsets')
    check(args['out_bytes'], c['records'], 'records')
    assert args['used'][0] == total


def test_spill_unpack_refusals(gpu_ctx):
    c = ref.case(SPILL_REFUSAL_CASE)
    rows = len(c['l'])
    pool = dict(zip(('l', 'u', 'v', 'ncut', 'ids'), spill_pool(c, True)))
    args = dict(n=65, nv=67, kc=5, count=5, root_l=c['root_l'], root_u=c['root_u'], offsets=c['offsets'], in_bytes=c['records'],
                slot=c['slot'], pool_rows=rows, **pool)
    wrong = c['records'].copy()
    wrong[8:12].view(np.int32)[0] += 1                                  # the first record's diff count
    swapped = c['records'].copy()                                       # two diff columns of a record out of order
    r2 = next(r for r in range(5) if swapped[c['offsets'][r] + 8:c['offsets'][r] + 12].view(np.int32)[0] >= 2)
    col = swapped[c['offsets'][r2] + 16:c['offsets'][r2] + 24].view(np.int32)
    col[0], col[1] = int(col[1]), int(col[0])
    bad = [(dict(n=0), 'n, nv or pool_rows < 1'), (dict(nv=0), 'n, nv or pool_rows < 1'), (dict(pool_rows=0), 'n, nv or pool_rows < 1'),
           (dict(count=-1), 'count < 0'), (dict(kc=65), 'kc outside'), (dict(kc=-1), 'kc outside'),
           (with_entry(args, 'slot', 0, rows), 'slot outside'), (with_entry(args, 'slot', 1, -1), 'slot outside'),
           (dict(slot=None, pool_rows=4), 'slot outside'), (with_entry(args, 'slot', 2, int(c['slot'][0])), 'two equal slots'),
           (dict(in_bytes=wrong), 'disagrees with its header'), (with_entry(args, 'offsets', 0, 8), 'offsets[0]'),
           (with_entry(args, 'offsets', 1, 8), 'bad offsets'), (dict(in_bytes=swapped), 'diff columns must ascend'),
           (dict(root_l=None), 'null'), (dict(root_u=None), 'null'), (dict(offsets=None), 'null'), (dict(in_bytes=None), 'null'),
           (dict(l=None), 'null'), (dict(u=None), 'null'), (dict(v=None), 'null'), (dict(ncut=None), 'null'), (dict(ids=None), 'null')]
    raw_refusals(gpu_ctx, 'mipx_noderows_spill_unpack', args, list(pool), bad)
    want = ref.decode(c['root_l'], c['root_u'], c['offsets'], c['records'], c['slot'], *spill_pool(c, True))
    for k, w in zip(pool, want):
        check(args[k], w, k)


def test_spill_gather_rows_refusals(gpu_ctx):
    g = ref.case('gather-rows-n2-nv7')
    args = dict(n=2, nv=7, count=7, slot=g['slot'], src_rows=6, src_l=g['src_l'], src_u=g['src_u'], src_v=g['src_v'],
                l=g['l'].copy(), u=g['u'].copy(), v=g['v'].copy())
    raw_refusals(gpu_ctx, 'mipx_noderows_spill_gather_rows', args, ['l', 'u', 'v'], [
        (dict(n=0), 'n, nv or src_rows < 1'), (dict(nv=0), 'n, nv or src_rows < 1'), (dict(src_rows=0), 'n, nv or src_rows < 1'),
        (dict(count=-1), 'count < 0'), (with_entry(args, 'slot', 1, 6), 'slot >= src_rows'), (dict(slot=None), 'null'),
        (dict(src_l=None), 'null'), (dict(src_u=None), 'null'), (dict(src_v=None), 'null'), (dict(l=None), 'null'), (dict(u=None), 'null'),
        (dict(v=None), 'null')])
    for k, w in zip('luv', ref.gather_rows_restated(g)):
        check(args[k], w, k)


@pytest.mark.parametrize('name', ref.GATHER_ROWS_CASES)
def test_spill_gather_rows_leaves_the_rows_on_the_host_alone(name, gpu_ctx):
    c = ref.case(name)
    got = [c[k].copy() for k in 'luv']
    _ffi.noderows_spill_gather_rows(gpu_ctx, c['n'], c['nv'], c['slot'], c['src_l'], c['src_u'], c['src_v'], *got)
    for g, w, k in zip(got, ref.gather_rows_restated(c), 'luv'):
        check(g, w, f'{name} {k}')
    assert all(np.all(g[c['slot'] < 0].view(np.uint8) == ref.FILL) for g in got)
