"""The exchange between the ranks of one search, pinned on one GPU in one process: the test IS the second rank
(tests/support/scripted_peer.py, written from include/mipx.h).  It reads every record and every donation the engine
emits and answers with records and messages built from the documentation alone; tests/test_scripted_peer_abi.py
checks without a GPU that the scripts played here reach the decisions they are named after.

A TWIN is a second tree on the same problem run through the same calls without a communicator: the engine is
deterministic, so the twin's open nodes are the state the rank under test is in.  test_own_records asserts first that
an idle scripted peer does not change a search.

All-gathers a case pins (x_tick / x_close of csrc/tree_engine.hip.h; every solve ends with the closing exchange):
  a dry rank              one per blocking exchange until the records say stop, + the closing one
  a rank at max_steps = 1 the one posted while its step runs, one per blocking exchange, + the closing one
"""
import collections

import numpy as np
import pytest

from simple_mip_solver_amd import _ffi
from simple_mip_solver_amd.generators import random_dense_milp_arrays
from tests.support import scripted_peer as sp

pytestmark = pytest.mark.gpu
INF = float('inf')
STORE = 1 << 20       # the default store_capacity
REGION = 1 << 14      # rows of the migration region in the cut-mode cases

Shape = collections.namedtuple('Shape', 'n m seed B MB target grow cut')
SMALL = Shape(40, 16, 3, 16, 512, 200, 16, None)
PAD = Shape(37, 15, 1, 8, 512, 120, 8, None)                 # (n + m) % 8 = 4: the pad behind the codes
WIDE = Shape(260, 24, 0, 16, 128, 40, 16, None)               # n > 256: the row kernels stride twice; a few dozen nodes
CUTS = Shape(64, 32, 5, 16, 512, 300, 64, {})                # kc at its cap (64)
CUTS8 = Shape(64, 32, 5, 16, 512, 300, 64, dict(max_cuts_per_node=8))     # a lowered cap
SHAPES = dict(small=SMALL, pad=PAD, wide=WIDE, cuts=CUTS, cuts8=CUTS8)

_problems = {}


def problem(ctx, s):
    key = (s.n, s.m, s.seed, s.cut is not None)
    if key not in _problems:
        A, b, c, l, u, ints = random_dense_milp_arrays(s.n, s.m, density=1.0, seed=s.seed)
        if s.cut is not None:
            u = np.full(s.n, INF)      # unboxed: open nodes carry, gain and lose cut rows (test_cut_migration_gpu.py)
        prob = _ffi.Problem(ctx, A, b, c)
        if s.cut is None:
            # The first tree in anchor mode leaves the root's tableau with the PROBLEM (mipx_problem_set_anchor), and
            # every later tree on it starts from that anchor: same nodes, other pivots, costs that differ in the last
            # bits.  A twin must not be the first tree of its problem, so a throw-away tree solves the root here.
            first = _ffi.Tree(prob, ints, l, u, branch_rule='pseudo cost', max_batch=2, pool_capacity=1 << 10)
            first.set_anchor_mode(True)
            first.solve(mip_gap=0.0, frontier_batch=2, max_steps=1)
            first.close()
        _problems[key] = (prob, ints, l, u, c, 1000.0 * float(np.max(np.abs(A))))
    return _problems[key]


def new_tree(ctx, s, MB=None):
    prob, ints, l, u, _, mac = problem(ctx, s)
    MB = s.MB if MB is None else MB
    if s.cut is not None:
        return _ffi.Tree(prob, ints, l, u, branch_rule='pseudo cost', max_batch=MB, pool_capacity=1 << 15,
                         cut_params=dict(max_abs_coef=mac, **s.cut))
    t = _ffi.Tree(prob, ints, l, u, branch_rule='pseudo cost', max_batch=MB, pool_capacity=1 << 15)
    if MB > 1:
        t.set_anchor_mode(True)
        t.set_dive(True)
    return t


def grown(ctx, s, target=None):
    t = new_tree(ctx, s)
    st = t.stats()
    while st['open_nodes'] < (s.target if target is None else target):
        st = t.solve(mip_gap=0.0, frontier_batch=s.grow, max_steps=1)
        assert st['status'] == 4
    if s.cut is not None:
        t.set_cut_migration(REGION)
    return t


def kc_of(t):
    return max(0, _ffi.lib().mipx_tree_cut_rows_per_node(t._h)) if t.cuts else 0


def open_nodes(t):
    """Every open node as a tuple of bytes -- dual bound, l, u, the codes of the columns and shared rows; with cut
    rounds also the codes of its cut rows and their (pi, pi0) in list order -- and (ids, cut lists) beside."""
    N = t.stats()['open_nodes']
    L, U, V, D = t.peek_open(N)
    ids, ncut, lists, codes = t.peek_cuts(N)
    assert len(D) == len(ids) == N
    keys = [(D[k].tobytes(), L[k].tobytes(), U[k].tobytes(), V[k].tobytes()) for k in range(N)]
    own = [lists[k, :ncut[k]].copy() if t.cuts else np.zeros(0, np.int32) for k in range(N)]
    if t.cuts:
        flat = np.concatenate(own + [np.zeros(0, np.int32)])
        pi, pi0 = t.cut_rows(flat)
        at = 0
        for k in range(N):
            nc = int(ncut[k])
            keys[k] += (codes[k, :nc].tobytes(), pi[at:at + nc].tobytes(), pi0[at:at + nc].tobytes())
            at += nc
    return keys, [int(i) for i in ids], own


def message_keys(d, s, kc):
    """The same tuples for the records of a decoded message (the meaningful bytes only)."""
    nv = s.n + s.m
    keys = []
    for k in range(d['count']):
        key = (d['meta'][k, 0].tobytes(), d['l'][k].tobytes(), d['u'][k].tobytes(), d['codes'][k, :nv].tobytes())
        if kc:
            nc, li = int(d['ncut'][k]), d['lists'][k]
            key += (d['codes'][k, nv:nv + nc].tobytes(), d['tab_pi'][li].tobytes(), d['tab_pi0'][li].tobytes())
        keys.append(key)
    return keys


def traced_step(t, MB):
    """One traced step over the whole queue: open-node tuple -> (LP status, objective bits) of that node."""
    keys, ids, _ = open_nodes(t)
    assert len(ids) <= MB
    t.set_trace(True)
    t.solve(mip_gap=0.0, frontier_batch=MB, max_steps=1)
    tr = t.trace()
    seen = {int(i): (int(st), o.tobytes()) for i, st, o in zip(tr['node_id'], tr['status'], tr['objective'])}
    out = {}
    for key, i in zip(keys, ids):
        if i in seen:       # (a node whose bound an incumbent already cuts off is closed without an LP)
            assert out.setdefault(key, seen[i]) == seen[i]      # (equal records evaluate alike)
    assert len(out) > 0
    return out


def attach(ctx, t, s, name, **kw):
    case = sp.cases(s.n, B=s.B, kc=kc_of(t), region=REGION if t.cuts else 0, **kw)[name]
    peer = sp.ScriptedPeer(s.n, case.script, sends=case.sends)
    comm = peer.comm(_ffi, ctx)
    t.set_comm(comm, 1)
    return peer, comm, case


def table_bytes(t):
    return tuple(a.tobytes() for a in t.pseudo_cost_arrays())


# ---- 4.1 the rank's own records ------------------------------------------------------------------------------------
@pytest.mark.parametrize('path,B,steps', [('device finish, steps overlapped', 16, 12),
                                          ('device finish, steps overlapped', 8, 12),
                                          ('host finish (exact mode)', 1, 30)])
def test_own_records(gpu_ctx, path, B, steps):
    """An idle peer, an exchange at every step, the table empty at the start (so that strong-branching probes are
    deferred to the host: the scenario of ADVICE.md's first item).  A posted record never takes back a sample.

    Before x_fill_record posted the per-entry high-water mark, the times did dip under the device finish: at B = 16
    record 7 -> 8 column 6 left 5 -> 4 and column 38 left and right 1 -> 0; at B = 8 record 5 -> 6 column 29 right
    6 -> 4 and record 6 -> 7 column 31 left 5 -> 3; each recovered one or two records later.

    The SUMS are asserted non-negative only.  Every sample is a cost >= 0, yet the posted sums are not monotone: at
    B = 8 column 31 right goes 3.8949653511624858 -> 3.4071250644923787 from record 8 to 9 while its times go 8 -> 9.
    Presumably (read from the code, not measured) because a sample that counts without a cost weighs in with the
    running mean of the table it is applied to, and the host's table (deferred nodes, pc_update) and the device's
    version (pc_apply) are not the same table at that moment.
    Host finish here is the exact mode: with the trace on and steps overlapped a search depends on host timing (a
    2 ms step hook alone changes its costs, no communicator involved), so it has no twin."""
    trace = False
    s = SMALL._replace(B=B, MB=B)
    n = s.n
    out = []
    for with_peer in (True, False, False):
        t = new_tree(gpu_ctx, s)
        if trace:
            t.set_trace(True)
        if with_peer:
            peer, comm, case = attach(gpu_ctx, t, s, 'idle', steps=steps)
            base = t.pseudo_cost_arrays()
            assert t.exchange_record()[2] == t.stats()['open_nodes']
        st = t.solve(mip_gap=0.0, frontier_batch=B, max_steps=steps)
        out.append((st, t.pseudo_cost_arrays(), open_nodes(t)[0], t))
    (st, table, queue, t), (st_twin, table_twin, queue_twin, _), (st_again, table_again, queue_again, _) = out
    recs = np.array(peer.records)
    own_s, own_t = recs[:, 16 + n:16 + 3 * n], recs[:, 16 + 3 * n:]
    keys = ('evaluated_nodes', 'lp_solved', 'probes_solved', 'pivots', 'steps', 'open_nodes', 'primal_bound', 'status')
    same = lambda a, b: all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    print(f'{path}, B = {B}: {len(recs)} records, own samples at the end {int(own_t[-1].sum())}; against the twin: table '
          f'{"equal" if same(table, table_twin) else [int(np.sum(x != y)) for x, y in zip(table, table_twin)]}, counters '
          f'{[(k, st[k], st_twin[k]) for k in keys if st[k] != st_twin[k]]}, queue {queue == queue_twin}; two twins: table '
          f'{same(table_twin, table_again)}, counters {all(st_twin[k] == st_again[k] for k in keys)}, queue '
          f'{queue_twin == queue_again}')
    # the engine is deterministic: two runs without a communicator agree (what every twin of this file relies on)
    assert same(table_twin, table_again) and queue_twin == queue_again and all(st_twin[k] == st_again[k] for k in keys)
    assert np.array_equal(recs[:, 9], np.arange(len(recs)))                       # [9] counts the exchanges
    assert np.all(np.diff(recs[:, 4:8], axis=0) >= 0)                             # the counters never decrease
    assert recs[-1, 2] == st['open_nodes'] and np.all(recs[:, 2] >= 0)            # the closing record: nothing in flight
    assert np.all(recs[:, 1] <= recs[:, 12])
    down_t = np.argwhere(np.diff(own_t, axis=0) < 0)
    for step, e in down_t[:8]:
        print(f'  times dip: record {step} -> {step + 1}, entry {e} ({"lr"[e // n]} of column {e % n}): '
              f'{own_t[step, e]} -> {own_t[step + 1, e]}, sums {own_s[step, e]!r} -> {own_s[step + 1, e]!r}')
    down_s = np.argwhere(np.diff(own_s, axis=0) < 0)
    for step, e in down_s[:8]:
        print(f'  sums dip: record {step} -> {step + 1}, entry {e}: {own_s[step, e]!r} -> {own_s[step + 1, e]!r}, times '
              f'{own_t[step, e]} -> {own_t[step + 1, e]}')
    assert len(down_t) == 0, f'{len(down_t)} posted times went down'
    assert np.all(own_s >= 0)       # (not monotone: the docstring)
    if path.startswith('host'):
        assert len(down_s) == 0     # one table, one recurrence: there the sums only grow
    cl, cr, tl, tr = t.pseudo_cost_arrays()
    assert np.array_equal(np.concatenate([base[2], base[3]]) + own_t[-1].astype(np.int64), np.concatenate([tl, tr]))
    # the idle peer changed nothing: table, evaluated nodes, bounds and open nodes are the twin's, bit for bit
    assert same(table, table_twin)
    for k in keys:
        assert st[k] == st_twin[k], k
    assert queue == queue_twin
    g = t.global_stats()
    assert g['exchanges'] == len(recs) <= len(case.script) and g['nodes_sent'] == g['nodes_received'] == 0
    assert recs[-1, 3] == 2 and recs[-2, 3] == 2 and np.all(recs[:-2, 3] == 0)    # the quota, posted when reached
    assert not peer.sent and not peer.asked
    t.set_comm(None)
    comm.close()


# ---- 4.2 merging the peer's samples, isolated ----------------------------------------------------------------------
def dry_tree(ctx, s, MB=None):
    t = new_tree(ctx, s, MB)
    t.solve(mip_gap=0.0, frontier_batch=min(s.B, t.max_batch), max_steps=2)
    t.keep_shard(999983, 1000003)                                                   # nothing
    assert t.stats()['open_nodes'] == 0
    return t


@pytest.mark.parametrize('dip_at', [None, 3], ids=['monotone', 'dip and recover'])
@pytest.mark.parametrize('path', ['device finish', 'host finish'])
def test_merging_the_peers_samples(gpu_ctx, path, dip_at):
    """The rank is dry: it sits in the blocking exchange, runs no step, and its table changes by merges alone.
    K = 6 records of cumulative samples, the idle record that ends the search, the closing one: K + 2 all-gathers."""
    s, K = SMALL, 6
    n = s.n
    table, seq, hot = sp.merge_sequences(n, seed=11, K=K, dip_at=dip_at)
    t = dry_tree(gpu_ctx, s, MB=s.B if path == 'device finish' else 1)
    t.set_pseudo_cost_arrays(*table)
    peer, comm, case = attach(gpu_ctx, t, s, 'merge', samples=seq)
    st = t.solve(mip_gap=1e-4, frontier_batch=min(s.B, t.max_batch))
    assert len(peer.records) == K + 2 == len(case.script) == t.global_stats()['exchanges']
    assert st['evaluated_nodes'] == t.global_stats()['evaluated_nodes'] and t.global_stats()['open_nodes'] == 0
    recs = np.array(peer.records)
    assert np.all(recs[:, 2] == 0) and np.all(recs[:, 16 + n:] == 0)               # the rank ran no step of its own
    cl, cr, tl, tr = t.pseudo_cost_arrays()
    last = seq[-1][2 * n:].astype(np.int64)
    got_t = np.concatenate([tl, tr]).astype(np.int64)
    want_t = np.concatenate([table[2], table[3]]).astype(np.int64) + last
    print(f'{path}, {"dip" if dip_at else "monotone"}: merged times {got_t.sum()}, the table\'s + the peer\'s last record '
          f'{want_t.sum()}; on the dipped entries {got_t[hot].tolist()} against {want_t[hot].tolist()}')
    assert np.array_equal(got_t, want_t)                                           # the peer's last record, not more
    if path == 'device finish':
        ref = sp.merge_reference(*table, seq)
    else:
        ref = sp.sum_form_reference(*table, seq[-1])
    assert cl.tobytes() == ref[0].tobytes() and cr.tobytes() == ref[1].tobytes()
    assert np.array_equal(tl, ref[2]) and np.array_equal(tr, ref[3])
    # an entry exists exactly where a merge happened or one existed (the host's flags are not exported: the table's
    # dict lists the columns with times on either side)
    assert sorted(t.pseudo_costs()) == np.where(ref[4])[0].tolist()
    t.set_comm(None)
    comm.close()


def test_merged_table_reaches_the_device(gpu_ctx):
    """pc_merge itself: a rank at its step quota merges the peer's samples into the DEVICE table while it blocks; the
    next step scores its nodes from that table and snapshots it back.  A twin that is handed the same merged table
    through mipx_tree_set_pseudo_costs runs the same step: tables, counters and open nodes agree bit for bit."""
    s, K = SMALL, 6
    n = s.n
    _, seq, _ = sp.merge_sequences(n, seed=12, K=K)
    t, twin = grown(gpu_ctx, s), grown(gpu_ctx, s)
    work = [sp.make_record(n, dual=-INF, open_nodes=s.B, batch=s.B, samples=q) for q in seq]
    end = sp.calm(stop=2, samples=lambda p: seq[-1])
    peer = sp.ScriptedPeer(n, [sp.calm()] + work + [end, end])
    comm = peer.comm(_ffi, gpu_ctx)
    t.set_comm(comm, 1)
    st = t.solve(mip_gap=0.0, frontier_batch=s.B, max_steps=1)
    twin.solve(mip_gap=0.0, frontier_batch=s.B, max_steps=1)
    assert len(peer.records) == K + 3 and st['status'] == 4
    t.set_comm(None)
    base = twin.pseudo_cost_arrays()
    ref = sp.merge_reference(*base, seq)
    assert table_bytes(t) == tuple(a.tobytes() for a in ref[:4])                   # the host mirror
    twin.set_pseudo_cost_arrays(*ref[:4])
    a = t.solve(mip_gap=0.0, frontier_batch=s.B, max_steps=2)
    b = twin.solve(mip_gap=0.0, frontier_batch=s.B, max_steps=2)
    assert table_bytes(t) == table_bytes(twin)                                     # the device table, two steps later
    assert all(a[k] == b[k] for k in ('evaluated_nodes', 'lp_solved', 'probes_solved', 'pivots', 'open_nodes'))
    assert open_nodes(t)[0] == open_nodes(twin)[0]
    comm.close()


# ---- 4.3 incumbents and termination through the real engine --------------------------------------------------------
@pytest.fixture(scope='module')
def plain(gpu_ctx):
    """The plain search of the small instance, run to the end: optimum, solution, evaluated nodes, steps."""
    t = new_tree(gpu_ctx, SMALL, MB=SMALL.B)
    st = t.solve(mip_gap=0.0, frontier_batch=SMALL.B)
    assert st['status'] == 1 and st['open_nodes'] == 0
    return dict(opt=st['primal_bound'], x=t.solution(), evaluated=st['evaluated_nodes'], steps=st['steps'])


def solved_tree(ctx, plain):
    t = new_tree(ctx, SMALL, MB=SMALL.B)
    st = t.solve(mip_gap=0.0, frontier_batch=SMALL.B)
    assert st['open_nodes'] == 0 and st['primal_bound'] == plain['opt'] and t.solution().tobytes() == plain['x'].tobytes()
    return t


def test_adopting_the_peers_incumbent(gpu_ctx, plain):
    s = SMALL
    t = new_tree(gpu_ctx, s, MB=s.B)
    peer, comm, case = attach(gpu_ctx, t, s, 'adopt', opt=plain['opt'], x=plain['x'])
    assert plain['steps'] + 4 <= len(case.script)
    st = t.solve(mip_gap=0.0, frontier_batch=s.B)
    recs = np.array(peer.records)
    assert st['status'] == 1 and st['primal_bound'] == plain['opt']
    assert t.solution().tobytes() == plain['x'].tobytes()                          # the peer's vector, bit for bit
    assert st['evaluated_nodes'] < plain['evaluated']                              # the incumbent did prune
    # the rank posts the adopted point as its own from the next record on: value, flag and vector
    assert recs[0, 8] == 0 and recs[0, 0] == INF
    assert np.all(recs[1:, 8] == 1) and np.all(recs[1:, 0] == plain['opt']) and np.all(recs[1:, 16:16 + s.n] == plain['x'])
    g = t.global_stats()
    # (mipx_exchange_decide: the LOWEST rank that holds a solution for the best value -- rank 0 since it adopted it)
    assert g['incumbent_rank'] == 0 and g['exchanges'] == len(recs) and np.array_equal(recs[:, 9], np.arange(len(recs)))
    assert recs[-1, 2] == 0 and recs[-2, 2] == 0                                   # decided idle, then the closing one
    t.set_comm(None)
    comm.close()


def test_adopting_at_the_closing_exchange(gpu_ctx, plain):
    """What the peer found since its last record arrives with the closing exchange: value, vector, and rank 1 holds it."""
    s = SMALL
    t = dry_tree(gpu_ctx, s, MB=s.B)
    peer, comm, case = attach(gpu_ctx, t, s, 'adopt_at_close', opt=plain['opt'], x=plain['x'])
    st = t.solve(mip_gap=0.0, frontier_batch=s.B)
    assert len(peer.records) == 2 == len(case.script)
    assert st['primal_bound'] == plain['opt'] and st['has_solution'] == 1
    assert t.solution().tobytes() == plain['x'].tobytes()
    assert t.global_stats()['incumbent_rank'] == 1
    t.set_comm(None)
    comm.close()


def test_incumbent_tie_keeps_the_own_solution(gpu_ctx, plain):
    s = SMALL
    t = solved_tree(gpu_ctx, plain)
    peer, comm, case = attach(gpu_ctx, t, s, 'tie', opt=plain['opt'], x=plain['x'])
    st = t.solve(mip_gap=0.0, frontier_batch=s.B)
    assert len(peer.records) == 2 == len(case.script)
    assert np.all(np.array(peer.records)[:, 8] == 1)
    assert st['status'] == 1 and st['primal_bound'] == plain['opt']
    assert t.solution().tobytes() == plain['x'].tobytes() and t.global_stats()['incumbent_rank'] == 0
    t.set_comm(None)
    comm.close()


@pytest.mark.parametrize('name,status', [('limit', 4), ('failure', None)])
def test_peer_limit_and_failure(gpu_ctx, name, status):
    s = SMALL
    t = dry_tree(gpu_ctx, s, MB=s.B)
    peer, comm, case = attach(gpu_ctx, t, s, name)
    if status is None:
        with pytest.raises(_ffi.MipxError, match='MIPX_EPEER|another rank failed'):
            t.solve(mip_gap=0.0, frontier_batch=s.B)
    else:
        assert t.solve(mip_gap=0.0, frontier_batch=s.B)['status'] == status
    # the blocking exchange that goes on, the one with the flag, the closing one
    assert len(peer.records) == 3 == len(case.script) == t.global_stats()['exchanges']
    t.set_comm(None)
    comm.close()


def test_global_gap_keeps_a_closed_rank_waiting(gpu_ctx, plain):
    s = SMALL
    t = solved_tree(gpu_ctx, plain)
    peer, comm, case = attach(gpu_ctx, t, s, 'gap', opt=plain['opt'], x=plain['x'])
    st = t.solve(mip_gap=1e-4, frontier_batch=s.B)
    recs = np.array(peer.records)
    # two exchanges with the peer's bound below, the one where it rises (reason 3), the closing one
    assert len(recs) == 4 == len(case.script) and np.all(recs[:, 2] == 0) and np.all(recs[:, 0] == plain['opt'])
    assert st['status'] == 1 and st['dual_bound'] == plain['opt'] and t.global_stats()['open_nodes'] == 1
    t.set_comm(None)
    comm.close()


def test_both_ranks_at_their_step_quota(gpu_ctx):
    s = SMALL
    t = grown(gpu_ctx, s)
    peer, comm, case = attach(gpu_ctx, t, s, 'quotas')
    st = t.solve(mip_gap=0.0, frontier_batch=s.B, max_steps=1)
    recs = np.array(peer.records)
    assert len(recs) == 3 == len(case.script) and recs[:, 3].tolist() == [0, 2, 2]
    assert recs[0, 2] >= s.B and np.isfinite(recs[0, 12]) and recs[1, 12] == INF     # in flight, then not
    assert st['status'] == 4 and t.global_stats()['exchanges'] == 3
    t.set_comm(None)
    comm.close()


# ---- 4.4 donor / 4.5 receiver / 4.6 cut mode -----------------------------------------------------------------------
def check_meta(d, s, ints):
    for k in range(d['count']):
        dual, b_val, depth, b_idx, b_dir = d['meta'][k, :5]
        assert depth >= 1 and depth == int(depth) and b_idx == int(b_idx) and int(b_idx) in ints and b_dir in (0.0, 1.0)
        j = int(b_idx)
        if b_dir == 0.0:
            assert d['u'][k, j] == np.floor(b_val), (k, j, b_val, d['u'][k, j])
        else:
            assert d['l'][k, j] == np.ceil(b_val), (k, j, b_val, d['l'][k, j])


def donate(ctx, s, name='donor', **kw):
    """The donor at its step quota against the scripted peer, and its twin.  Returns everything the assertions need."""
    t, twin = grown(ctx, s), grown(ctx, s)
    peer, comm, case = attach(ctx, t, s, name, **kw)
    t.solve(mip_gap=0.0, frontier_batch=s.B, max_steps=1)
    twin.solve(mip_gap=0.0, frontier_batch=s.B, max_steps=1)
    assert len(peer.records) == 4 == len(case.script) and not peer.asked
    return t, twin, peer, comm


_donations = {}


def donation(ctx, shape):
    """The donor case of a shape, asserted once and kept for the receiver cases: the decoded message, the sizes, and
    what one traced step of the twin makes of every open node."""
    if shape in _donations:
        return _donations[shape]
    s = SHAPES[shape]
    n = s.n
    t, twin, peer, comm = donate(ctx, s)
    kc = kc_of(t)
    nvs = n + s.m + kc
    mine, reply = sp.parse_record(peer.records[1], n), sp.parse_record(peer.replies[1], n)
    amount = sp.hand_amount(mine['open_nodes'], reply['open_nodes'], reply['room'])
    ctab = sp.table_rows(reply['region_free'], amount, kc)
    if kc:
        assert (mine['region_free'], mine['kc'], mine['cut_rounds']) == (REGION, kc, 1)
    else:
        assert (mine['region_free'], mine['kc'], mine['cut_rounds']) == (0, 0, 0)
    assert len(peer.sent) == 1 and len(peer.sent[0]) == sp.layout(n, nvs, amount, kc, ctab).bytes
    d = sp.decode_message(peer.sent[0], n, nvs, amount, kc, ctab)
    before, _, lists_before = open_nodes(twin)
    N = len(before)
    assert mine['open_nodes'] == N and mine['stop'] == 2
    give = min(amount, (N - s.B) // 2)
    assert give > 0 and d['count'] == give
    check_meta(d, s, problem(ctx, s)[1])
    sent = message_keys(d, s, kc)
    have, gone = collections.Counter(before), collections.Counter(sent)
    assert not gone - have                                                         # each one of the twin's, at most once
    after, _, _ = open_nodes(t)
    assert collections.Counter(after) == have - gone                               # and they left the donor's queue
    g = t.global_stats()
    assert g['nodes_sent'] == give and g['nodes_received'] == 0
    if kc:
        # every distinct store id of the donated nodes is one table row: refs <-> store ids one to one
        by_key = collections.defaultdict(list)
        for key, li in zip(before, lists_before):
            by_key[key].append(li)
        ref_of = {}
        for k, key in enumerate(sent):
            ids = by_key[key].pop()
            assert len(ids) == d['ncut'][k]
            for r, i in zip(d['lists'][k].tolist(), ids.tolist()):
                assert ref_of.setdefault(i, r) == r
        assert sorted(ref_of.values()) == list(range(d['rows_used'])) and d['rows_used'] > 0
        cm = t.cut_migration_stats()
        assert cm['cut_rows_sent'] == d['rows_used'] and cm['nodes_sent_with_cuts'] == int(np.sum(d['ncut'] > 0)) > 0
    t.set_comm(None)
    comm.close()
    out = dict(d=d, amount=amount, ctab=ctab, kc=kc, nvs=nvs, keys=sent, outcome=traced_step(twin, s.MB))
    _donations[shape] = out
    return out


@pytest.mark.parametrize('shape', list(SHAPES))
def test_donor(gpu_ctx, shape):
    s = SHAPES[shape]
    if shape == 'wide':
        assert _ffi.kernel_name(s.m, s.n)                                          # the shape dispatches
    don = donation(gpu_ctx, shape)
    print(f'{shape}: amount {don["amount"]}, count {don["d"]["count"]}, {len(don["outcome"])} open nodes in the twin, '
          f'kc {don["kc"]}, table rows {don["d"].get("rows_used")} of {don["ctab"]}')


@pytest.mark.parametrize('shape', ['small', 'cuts'])
def test_donor_capped_by_the_receivers_room(gpu_ctx, shape):
    s = SHAPES[shape]
    n = s.n
    t, twin, peer, comm = donate(gpu_ctx, s, room=3)
    kc = kc_of(t)
    nvs = n + s.m + kc
    ctab = sp.table_rows(REGION if kc else 0, 3, kc)
    assert len(peer.sent) == 1 and len(peer.sent[0]) == sp.layout(n, nvs, 3, kc, ctab).bytes
    d = sp.decode_message(peer.sent[0], n, nvs, 3, kc, ctab)
    assert d['count'] == 3 == t.global_stats()['nodes_sent']
    have, gone = collections.Counter(open_nodes(twin)[0]), collections.Counter(message_keys(d, s, kc))
    assert not gone - have and collections.Counter(open_nodes(t)[0]) == have - gone
    t.set_comm(None)
    comm.close()


@pytest.mark.parametrize('shape', ['small', 'cuts'])
def test_no_move_between_equal_ranks(gpu_ctx, shape):
    s = SHAPES[shape]
    t, twin, peer, comm = donate(gpu_ctx, s, name='no_move')
    assert not peer.sent and t.global_stats()['nodes_sent'] == 0
    assert collections.Counter(open_nodes(t)[0]) == collections.Counter(open_nodes(twin)[0])
    t.set_comm(None)
    comm.close()


def test_donor_keeps_nodes_whose_rows_do_not_fit(gpu_ctx):
    """Cut mode, a peer whose region takes 3 rows: candidates whose rows no longer fit the table stay in the queue."""
    s = CUTS
    n = s.n
    t, twin, peer, comm = donate(gpu_ctx, s, peer_region=3)
    kc = kc_of(t)
    nvs = n + s.m + kc
    mine, reply = sp.parse_record(peer.records[1], n), sp.parse_record(peer.replies[1], n)
    amount = sp.hand_amount(mine['open_nodes'], reply['open_nodes'], reply['room'])
    assert sp.table_rows(reply['region_free'], amount, kc) == 3
    assert len(peer.sent[0]) == sp.layout(n, nvs, amount, kc, 3).bytes
    d = sp.decode_message(peer.sent[0], n, nvs, amount, kc, 3)
    before = open_nodes(twin)[0]
    assert 0 < d['count'] < min(amount, (len(before) - s.B) // 2) and 0 <= d['rows_used'] <= 3
    have, gone = collections.Counter(before), collections.Counter(message_keys(d, s, kc))
    assert not gone - have and collections.Counter(open_nodes(t)[0]) == have - gone       # nothing lost
    assert t.global_stats()['nodes_sent'] == d['count']
    t.set_comm(None)
    comm.close()


def receiver(ctx, s):
    """A rank that keeps one node of the grown tree and does its one step: at its quota with a few nodes."""
    t = grown(ctx, s)
    t.keep_shard(0, 10 ** 6)
    assert t.stats()['open_nodes'] == 1
    return t


def table_of(don, take):
    """The cut table of the first `take` donated records alone: their refs renumbered in the order of first use."""
    d = don['d']
    new, lists = {}, []
    for li in d['lists'][:take]:
        lists.append(np.array([new.setdefault(int(r), len(new)) for r in li], np.int32))
    rows = np.array(sorted(new, key=new.get), np.int64)
    return lists, d['tab_pi'][rows], d['tab_pi0'][rows]


def build_message(don, s, k, take, lists=None, **kw):
    d, kc = don['d'], don['kc']
    cut = {}
    if kc:
        own_lists, pi, pi0 = table_of(don, take)
        cut = dict(kc=kc, ctab=sp.table_rows(REGION, take, kc), lists=(own_lists if lists is None else lists)[:k],
                   tab_pi=pi, tab_pi0=pi0)
    cut.update(kw)
    return sp.encode_message(s.n, don['nvs'], take, d['l'][:k], d['u'][:k], d['codes'][:k], d['meta'][:k], **cut)


@pytest.mark.parametrize('part', ['all', 'some', 'none'])
@pytest.mark.parametrize('shape', list(SHAPES))
def test_receiver(gpu_ctx, shape, part):
    s = SHAPES[shape]
    n = s.n
    don = donation(gpu_ctx, shape)
    kc = don['kc']
    take = min(40, don['d']['count'])
    k = dict(all=take, some=take * 5 // 8, none=0)[part]
    if kc:
        tab_lists, tab_pi, tab_pi0 = table_of(don, take)
        assert 0 < len(tab_pi0) <= sp.table_rows(REGION, take, kc)
    t, twin = receiver(gpu_ctx, s), receiver(gpu_ctx, s)
    peer, comm, case = attach(gpu_ctx, t, s, 'receiver', take=take)
    peer.push(build_message(don, s, k, take))
    t.solve(mip_gap=0.0, frontier_batch=s.B, max_steps=1)
    twin.solve(mip_gap=0.0, frontier_batch=s.B, max_steps=1)
    assert len(peer.records) == 4 == len(case.script) and not peer.sent
    mine, reply = sp.parse_record(peer.records[1], n), sp.parse_record(peer.replies[1], n)
    assert sp.hand_amount(reply['open_nodes'], mine['open_nodes'], mine['room']) == take
    ctab = sp.table_rows(mine['region_free'], take, kc)
    # a real donor sends exactly that many bytes: a mismatch here is a deadlock between real ranks
    assert peer.asked == [(1, sp.layout(n, don['nvs'], take, kc, ctab).bytes)]
    own, _, _ = open_nodes(twin)
    got, ids, lists = open_nodes(t)
    assert collections.Counter(got) == collections.Counter(own) + collections.Counter(don['keys'][:k])
    g = t.global_stats()
    assert g['nodes_received'] == k and g['nodes_sent'] == 0
    assert sp.parse_record(peer.records[2], n)['open_nodes'] == len(own) + k
    if kc:
        used = len(tab_pi0) if k else 0
        cm = t.cut_migration_stats()
        assert cm['cut_rows_received'] == used == cm['region_rows_used']
        base = STORE - REGION
        if k:   # the rows land at the region base in table order, the lists point at them
            pi, pi0 = t.cut_rows(np.arange(base, base + used))
            assert pi.tobytes() == tab_pi.tobytes() and pi0.tobytes() == tab_pi0.tobytes()
            arrived = sorted(ids)[len(own):]                                       # (migrated nodes get new ids)
            by_id = dict(zip(ids, lists))
            assert [by_id[i].tolist() for i in arrived] == [(base + li).tolist() for li in tab_lists[:k]]
    t.set_comm(None)
    comm.close()
    if k:       # one traced step: the received nodes evaluate as the donor's twin evaluated them
        mine_out = traced_step(t, s.MB)
        both = [key for key in don['keys'][:k] if key in mine_out and key in don['outcome']]
        assert len(both) > 0 and (len(both) == k or np.isfinite(t.stats()['primal_bound']))
        for key in both:
            assert mine_out[key] == don['outcome'][key]


@pytest.mark.parametrize('shape', ['small', 'cuts'])
@pytest.mark.parametrize('count', [-1, 'amount + 1'])
def test_receiver_refuses_a_corrupt_count(gpu_ctx, shape, count):
    s = SHAPES[shape]
    don = donation(gpu_ctx, shape)
    take = min(40, don['d']['count'])
    t, twin = receiver(gpu_ctx, s), receiver(gpu_ctx, s)
    peer, comm, case = attach(gpu_ctx, t, s, 'receiver', take=take)
    peer.push(build_message(don, s, take, take, count=-1 if count == -1 else take + 1))
    with pytest.raises(_ffi.MipxError, match='corrupt migration message'):
        t.solve(mip_gap=0.0, frontier_batch=s.B, max_steps=1)
    twin.solve(mip_gap=0.0, frontier_batch=s.B, max_steps=1)
    assert len(peer.records) == 2 and len(peer.asked) == 1
    assert open_nodes(t)[0] == open_nodes(twin)[0] and t.global_stats()['nodes_received'] == 0     # unchanged
    t.set_comm(None)
    comm.close()


def test_receiver_refuses_a_ref_outside_the_table(gpu_ctx):
    s = CUTS
    don = donation(gpu_ctx, 'cuts')
    d = don['d']
    take = min(40, d['count'])
    lists, _, tab_pi0 = table_of(don, take)
    victim = next(k for k in range(take) if len(lists[k]) > 0)
    lists[victim][-1] = len(tab_pi0)                                               # the first row outside
    t = receiver(gpu_ctx, s)
    peer, comm, case = attach(gpu_ctx, t, s, 'receiver', take=take)
    peer.push(build_message(don, s, take, take, lists=lists))
    with pytest.raises(_ffi.MipxError, match='corrupt cut lists'):
        t.solve(mip_gap=0.0, frontier_batch=s.B, max_steps=1)
    # cutmig_unpack_lists counted it and wrote nothing through it: that node has no cut row, no list points outside
    _, _, own = open_nodes(t)
    base = STORE - REGION
    assert all(np.all((li < base) | ((li >= base) & (li < base + len(tab_pi0)))) for li in own)
    t.set_comm(None)
    comm.close()
