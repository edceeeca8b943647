"""The six kernels of a cut round (csrc/tree_kernels.hip.h, csrc/cut_kernels.hip.h) on synthetic rounds, through
mipx_cut_round_begin_batch and mipx_cut_round_generate_batch (include/mipx_cutround.h: the same launches as the
engine's, enqueue_cut_begin and enqueue_cut_generate), against the plain restatement of the reference's loop in
tests/support/cut_round_reference.py -- at every workgroups-per-node and group size of K2, odd and even shapes, both
right-hand-side folds, full slabs, lists and stores, pools with holes, and the edges of the stall test and the slack-cut
removal.  Nothing here is a tolerance: every comparison is of bits.  The one thing compared THROUGH the store ids and
not as ids is which node got which id with B > 1 (an atomicAdd across workgroups decides)."""
import numpy as np
import pytest

from tests.support import cut_round_reference as ref

pytestmark = pytest.mark.gpu
FILL = 0x5a
F = ref.F
IN_OUT = ('vstat', 'ncut', 'ids', 'state', 'pool_list', 'slab_pi', 'slab_pi0', 'store_pi', 'store_pi0', 'store_count', 'resolve',
          'counters')


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def untouched(a):
    return bool(np.all(np.ascontiguousarray(a).view(np.uint8) == FILL))


_PROBLEMS = {}


def problem_of(ctx, name, s):
    from simple_mip_solver_amd import _ffi
    if name not in _PROBLEMS:
        _PROBLEMS[name] = _ffi.Problem(ctx, s['A'], s['b'], np.zeros(s['A'].shape[1]))
    return _PROBLEMS[name]


def check_begin(s, got, want):
    for k in ('vstat', 'ncut', 'ids', 'state', 'obj_before', 'active', 'counters', 'resolve', 'need_tab'):
        assert same_bits(got[k], want[k].astype(got[k].dtype)), k
    # counters[1] is not begin's; counters[2] only the gather's
    assert got['counters'][1] == s['counters'][1]
    if not s['gather']:
        assert got['counters'][2] == s['counters'][2]
        # what lies past a node's new list is what lay there before
        for k in range(s['B']):
            nc = int(got['ncut'][k])
            assert same_bits(got['ids'][k, nc:], np.asarray(s['ids'], np.int32).reshape(s['B'], -1)[k, nc:])
    assert same_bits(got['vstat'][:, :s['n'] + s['m0']], np.asarray(s['vstat'], np.int8)[:, :s['n'] + s['m0']])


@pytest.mark.parametrize('name', ref.BEGIN_CASES)
def test_begin_equals_the_restatement(gpu_ctx, name):
    from simple_mip_solver_amd import _ffi
    s, want = ref.case(name)
    check_begin(s, _ffi.cut_round_begin_batch(gpu_ctx, s, fill=FILL), want)


def check_generate(s, got, want, exact_ids):
    """got against the restatement.  exact_ids: one valid order of the store ids is THE order (one node takes them
    all); otherwise everything that depends on who got which id is compared through the ids."""
    B, kc, cap = s['B'], s['kc'], s['store_cap']
    m0, n = s['A'].shape
    count0 = int(s['store_count'][0])
    for k in range(B):
        if not s['active'][k]:
            # a node that does not generate: nothing of it is written
            for key in ('k2_ncuts', 'k3_nadded', 'k3_added', 'k3_term'):
                assert untouched(got[key][k]), (key, k)
            for key in ('vstat', 'ncut', 'ids', 'pool_list', 'slab_pi', 'slab_pi0', 'resolve'):
                assert same_bits(got[key][k], np.asarray(s[key])[k].astype(got[key].dtype)), (key, k)
            assert same_bits(got['state'][:, k], np.asarray(s['state'], np.int32)[:, k])
            continue
        nadd = want['k3_nadded'][k]
        assert got['k2_ncuts'][k] == want['k2_ncuts'][k] and got['k3_nadded'][k] == nadd and got['k3_term'][k] == want['k3_term'][k], k
        assert got['k3_added'][k, :nadd].tolist() == want['k3_added'][k] and untouched(got['k3_added'][k, nadd:]), k
    # the slabs and the pools: no id in them
    for key in ('slab_pi', 'slab_pi0', 'pool_list'):
        assert same_bits(got[key], want[key]), key
    racy = not exact_ids and want['store_room'] < want['attempts']       # the store fills up part way through B > 1 nodes
    fields = [f for f in ref.FIELDS if not (racy and f in ('ncut_out', 'dropped'))]
    for f in fields:
        assert same_bits(got['state'][F[f]], want['state'][F[f]]), f
    if not racy:
        assert got['store_count'][0] == count0 + want['attempts']        # (every attempt counts, also past the cap)
    assert got['counters'][0] == s['counters'][0] and got['counters'][3] == s['counters'][3]
    if exact_ids:
        for key in IN_OUT:
            assert same_bits(got[key], want[key]), key
        return
    # ---- through the ids ----
    new_ids, attempts = [], 0
    for k in range(B):
        p = want['per_node'][k]
        if p is None:
            continue
        nc = int(got['ncut'][k])
        mine = got['ids'][k, p['nc0']:nc]
        took = len(mine)
        new_ids += mine.tolist()
        # a node asks the store until its list is full: one that lost an entry (the ids only rise: every later one too)
        # has asked for its whole selection
        attempts += took if took == p['wanted'] else p['nadd']
        assert np.all(np.diff(mine) > 0), k                               # a node's ids rise
        assert same_bits(got['ids'][k, :p['nc0']], np.asarray(s['ids'], np.int32)[k, :p['nc0']])
        assert same_bits(got['ids'][k, nc:], np.asarray(s['ids'], np.int32)[k, nc:])           # (the tail stays)
        # the node keeps a prefix of its selection, in order
        assert took <= p['wanted'] and (racy or took == p['wanted']), k
        assert same_bits(got['store_pi'][mine], p['selected_pi'][:took]) and same_bits(got['store_pi0'][mine], p['selected_pi0'][:took]), k
        vs = np.array(s['vstat'][k], np.int8)
        vs[n + m0 + p['nc0']:n + m0 + nc] = 1
        assert same_bits(got['vstat'][k], vs), k
        assert got['state'][F['ncut_out'], k] == nc
        assert got['state'][F['dropped'], k] == s['state'][F['dropped'], k] + p['k2_dropped'] + p['nadd'] - took, k
        assert got['resolve'][k] == int(bool(p['resolve_in']) or took > 0), k
    assert got['store_count'][0] == count0 + attempts
    total = min(attempts, want['store_room'])
    assert sorted(new_ids) == list(range(count0, count0 + total))          # exactly the ids handed out, each once
    rest = np.setdiff1d(np.arange(cap), new_ids)
    assert same_bits(got['store_pi'][rest], np.asarray(s['store_pi'])[rest]) and same_bits(got['store_pi0'][rest], np.asarray(s['store_pi0'])[rest])
    active = [k for k in range(B) if s['active'][k]]
    assert got['counters'][1] == s['counters'][1] + int(np.sum(got['resolve'][active] != 0))
    assert got['counters'][2] == max(int(s['counters'][2]), int(got['ncut'][active].max()))
    if racy:
        dropped_now = got['state'][F['dropped']] - np.asarray(s['state'], np.int32)[F['dropped']]
        asked = sum(p['k2_dropped'] + p['nadd'] for p in want['per_node'] if p)
        # the prefixes sum to the room that was left, the dropped counts to the rest
        assert len(new_ids) == want['store_room'] and int(dropped_now.sum()) == asked - want['store_room']


def exact(s, want):
    return sum(1 for p in want['per_node'] if p and p['wanted']) <= 1


@pytest.mark.parametrize('name', [c for c in ref.GENERATE_CASES if c not in ref.SWEEP_CASES])
def test_generate_equals_the_restatement(gpu_ctx, name):
    from simple_mip_solver_amd import _ffi
    s, want = ref.case(name)
    got = _ffi.cut_round_generate_batch(problem_of(gpu_ctx, name, s), s, fill=FILL)
    if s['B'] == 1:
        assert exact(s, want)                # (the store-full edge is exact with one node)
    check_generate(s, got, want, exact(s, want))
    if name == 'generate-fold-1024x512-above-64KiB':
        assert (got['chunks'], got['group']) == (16, 8)     # the engine's own rule: 116 KiB of LDS a workgroup


@pytest.mark.parametrize('name', ref.SWEEP_CASES)
def test_every_launch_shape_gives_the_same_bits(gpu_ctx, name):
    """K2 at 1, 4 and 16 workgroups a node and groups of 1, 3, 7 and 8 cuts: per cut the arithmetic and its order do not
    depend on either -- at n = 64, m = 32 the loop of a full group runs, at 65 x 33 (n odd) and 64 x 33 (n + ms odd) its
    guarded fallback does, as it does for every group below 8."""
    from simple_mip_solver_amd import _ffi
    s, want = ref.case(name)
    p = problem_of(gpu_ctx, name, s)
    first = None
    for chunks in (1, 4, 16):
        for group in (1, 3, 7, 8):
            got = _ffi.cut_round_generate_batch(p, dict(s, chunks=chunks, group=group), fill=FILL)
            assert (got['chunks'], got['group']) == (chunks, group)
            check_generate(s, got, want, exact(s, want))
            # ... and what does not depend on the ids is the same bytes from launch to launch
            if first is None:
                first = got
            for key in ('slab_pi', 'slab_pi0', 'pool_list', 'k2_ncuts', 'k3_nadded', 'k3_added', 'k3_term', 'ncut', 'state', 'store_count'):
                assert same_bits(got[key], first[key]), (chunks, group, key)


def test_two_rounds_in_a_row(gpu_ctx, oracle):
    """begin -> generate -> begin -> generate on one state: the second round's inputs are the first round's outputs, so
    that the two entries cannot disagree about what a field means.  Between the rounds the test supplies what the LP
    launches would: new duals (two of the new rows slack), objectives and tableaux."""
    from simple_mip_solver_amd import _ffi
    n, m, kc, B = 21, 10, 8, 3
    g = ref._blank(n, m, kc, B, 2024, (2, 0, 1), slab_rows=3 * (m + kc), store_used=10)
    g['is_int'][:] = 1
    p = _ffi.Problem(gpu_ctx, g['A'], g['b'], np.zeros(n))
    rng = np.random.default_rng(5)
    b = dict(n=n, m0=m, kc=kc, B=B, round=0, max_rounds=5, progress_tol=ref.TOL, max_dual_bound=ref.INF, have_dump=1, gather=0,
             status=np.zeros(B, np.int32), obj=np.array([3.0, 4.0, 5.0]), mipf=np.zeros(B, np.int32), y=rng.uniform(0.5, 1.0, (B, m + kc)),
             vstat=g['vstat'], ncut=g['ncut'], ids=g['ids'], state=np.zeros((len(ref.FIELDS), B), np.int32), obj_before=np.zeros(B),
             active=np.zeros(B, np.int32), counters=np.zeros(4, np.int32))
    b['y'][0, m] = 0.0                                   # node 0 starts by losing its first cut row
    taken = []
    for rnd in range(2):
        b['round'] = rnd
        want_b, got_b = ref.begin(b), _ffi.cut_round_begin_batch(gpu_ctx, b, fill=FILL)
        check_begin(b, got_b, want_b)
        assert got_b['active'].tolist() == [1, 1, 1]
        # the tableaux of the bases the nodes now have (any split with the node's number of rows will do for K2)
        parts = [ref._tableau(rng, n, m + int(got_b['ncut'][k]), m + kc, g['is_int']) for k in range(B)]
        for k in range(B):
            basic = parts[k][1][n:n + m + int(got_b['ncut'][k])]
            got_b['vstat'][k, :n + m + int(got_b['ncut'][k])] = 0
            got_b['vstat'][k, basic] = 1
        g.update(T=np.stack([q[0] for q in parts]), idx=np.stack([q[1] for q in parts]), x=np.stack([q[3] for q in parts]),
                 active=got_b['active'], vstat=got_b['vstat'], ncut=got_b['ncut'], ids=got_b['ids'], state=got_b['state'],
                 resolve=got_b['resolve'], counters=got_b['counters'])
        want_g = ref.generate(g, oracle)
        got_g = _ffi.cut_round_generate_batch(p, g, fill=FILL)
        check_generate(g, got_g, want_g, False)
        taken.append(int(got_g['store_count'][0]))
        # the next round: the first one's outputs, and what the re-solve would bring
        g.update({key: got_g[key] for key in IN_OUT})
        g['counters'][:2] = 0
        g['counters'][3] = 0
        y = rng.uniform(0.5, 1.0, (B, m + kc))
        for k in range(B):
            if got_g['ncut'][k] >= 2:
                y[k, m + int(got_g['ncut'][k]) - 2] = 0.0          # a row added in round 0 is slack in round 1
        b.update(y=y, obj=b['obj'] + 1.0, vstat=got_g['vstat'], ncut=got_g['ncut'], ids=got_g['ids'], state=got_g['state'],
                 obj_before=got_b['obj_before'], active=got_b['active'], counters=g['counters'])
    st = got_g['state']
    assert st[F['rounds']].tolist() == [2, 2, 2] and taken[1] >= taken[0] > 10
    assert np.all(st[F['n_created']] >= st[F['n_added']]) and int(st[F['n_removed']].sum()) >= 2


def test_entries_refuse_what_is_out_of_range(gpu_ctx):
    from simple_mip_solver_amd import _ffi
    L = _ffi.lib()
    buf = np.zeros(1 << 14, np.float64)
    p = _ffi._ptr(buf)
    scalars = dict(n=5, m0=3, kc=8, B=2, round=0, max_rounds=5, have_dump=1, gather=0, pool_rows=4)

    def call_begin(**change):
        v = dict(scalars, **change)
        return L.mipx_cut_round_begin_batch(gpu_ctx._h, v['n'], v['m0'], v['kc'], v['B'], v['round'], v['max_rounds'], 1e-4, 1e9, v['have_dump'],
                                            v['gather'], v['pool_rows'], *([p] * 16))
    assert call_begin() == 0                                     # (all zeros is a valid round)
    for change in (dict(B=0), dict(kc=0), dict(kc=65), dict(n=0), dict(n=1025), dict(m0=0), dict(round=-1), dict(max_rounds=-1), dict(have_dump=2),
                   dict(gather=2), dict(gather=1, pool_rows=0), dict(m0=190), dict(n=300, m0=1020)):
        assert call_begin(**change) == -1, change                # MIPX_EINVAL
    s, _ = ref.case('begin-gather-largest-last')
    for key, index, value in (('slot', 0, len(s['pool_ncut'])), ('slot', 4, -1), ('pool_ncut', 7, 65), ('pool_ncut', 1, -1)):
        bad = dict(s)
        bad[key] = np.array(s[key])
        bad[key][index] = value
        with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL'):
            _ffi.cut_round_begin_batch(gpu_ctx, bad)
    s, _ = ref.case('begin-B5-kc5-round0-dump1-gather0-off0')
    for value in (-1, 6):
        bad = dict(s, ncut=np.array(s['ncut']))
        bad['ncut'][3] = value
        with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*ncut'):
            _ffi.cut_round_begin_batch(gpu_ctx, bad)
    # generate: the scalars first, then every index a kernel would follow
    name = 'generate-k3-holes'
    s, _ = ref.case(name)
    prob = problem_of(gpu_ctx, name, s)
    for change in (dict(B=0), dict(kc=0), dict(kc=65), dict(slab_rows=0), dict(slab_rows=2041), dict(chunks=2), dict(chunks=-1), dict(chunks=32),
                   dict(group=-1), dict(group=9), dict(store_cap=0), dict(max_nonzero_coefs=0), dict(min_cut_depth=0.0), dict(max_term=0.0)):
        v = dict(s, **change)
        rc = L.mipx_cut_round_generate_batch(prob._h, v['B'], v['kc'], v['slab_rows'], v['chunks'], v['group'], v['store_cap'], v['max_term'],
                                             v['max_nonzero_coefs'], v['min_cut_depth'], v['cos_parallel'], v['max_abs_coef'], *([p] * 22))
        assert rc == -1, change
    n, m0 = s['A'].shape[1], s['A'].shape[0]
    edits = [('ncut', 0, 9, 'ncut'), ('ncut', 1, -1, 'ncut'), ('ids', (0, 0), s['store_cap'], 'id outside'), ('ids', (0, 0), -1, 'id outside'),
             ('pool_list', (0, 2), s['slab_rows'], 'pool_list'), ('pool_list', (1, 0), -1, 'pool_list'),
             ('state', (F['pool_n'], 0), s['slab_rows'] + 1, 'count'), ('state', (F['slab_n'], 1), -1, 'count'),
             ('state', (F['slab_n'], 1), s['slab_rows'] + 1, 'count'), ('state', (F['pool_n'], 1), int(s['state'][F['slab_n'], 1]) + 1, 'count'),
             ('store_count', 0, -1, 'store_count'), ('idx', (0, 0), n + m0 + 1, 'split'), ('idx', (0, 3), -1, 'split'),
             ('idx', (1, n + 1), int(s['idx'][1, 0]), 'split')]
    for key, index, value, what in edits:
        bad = dict(s)
        bad[key] = np.array(s[key])
        bad[key][index] = value
        with pytest.raises(_ffi.MipxError, match='MIPX_EINVAL.*' + what):
            _ffi.cut_round_generate_batch(prob, bad)
    # ... and the valid round still runs after all of that
    check_generate(s, _ffi.cut_round_generate_batch(prob, s, fill=FILL), ref.case(name)[1], exact(s, ref.case(name)[1]))
