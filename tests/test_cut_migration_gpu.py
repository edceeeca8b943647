"""Migration of open nodes with their cut rows in cut-round mode (include/mipx_cutmig.h), on one GPU.

mipx_tree_migrate_self sends open nodes of a tree with cut rounds through the communicator's point-to-point
path to its own rank (RCCL with the one rank a one-GPU box allows, or the custom transport): the nodes come
back under new ids, their cut rows in the tree's migration region.  Checked bit for bit: every open node's
bounds, basis codes (of the shared and the cut rows), inherited bound and cut rows (pi, pi0 in list order)
survive the trip, the region grows by the distinct rows moved, and one step over all open nodes evaluates
them exactly as the tree that moved nothing.  Also: the option's argument checks, the lowered cap of the
tree's own cuts, and a table too small for every node's rows."""
import numpy as np
import pytest

from simple_mip_solver_amd import _ffi
from simple_mip_solver_amd.generators import random_dense_milp_arrays

pytestmark = pytest.mark.gpu
INF = np.inf
STORE = 1 << 20     # the default store_capacity


def instance(ctx, n, m, seed):
    """The cut-carrying shapes of test_cut_rounds_gpu.py (unboxed: nodes carry, gain and lose cut rows)."""
    A, b, c, l, u, ints = random_dense_milp_arrays(n, m, density=1.0, seed=seed)
    u = np.full(n, INF)
    return _ffi.Problem(ctx, A, b, c), ints, l, u, 1000.0 * float(np.max(np.abs(A)))


def grown_tree(prob, ints, l, u, max_abs_coef, target, MB, **cut_params):
    t = _ffi.Tree(prob, ints, l, u, branch_rule='pseudo cost', max_batch=MB, pool_capacity=1 << 15,
                  cut_params=dict(max_abs_coef=max_abs_coef, **cut_params))
    st = t.stats()
    while st['open_nodes'] < target:
        st = t.solve(mip_gap=0.0, frontier_batch=64, max_steps=1)
        assert st['status'] == 4
    return t


def one_rank_comm(ctx, transport):
    if transport == 'rccl':
        comm = _ffi.Comm(ctx, 0, 1, unique_id=_ffi.comm_unique_id())
    else:
        comm = _ffi.Comm(ctx, 0, 1, allgather=lambda b: [b], send=lambda p, d: None, recv=lambda p, k: b'')
    assert comm.transport == transport
    return comm


def open_nodes(t, N):
    """Every open node as bytes: (dual bound, l, u, basis codes of the shared rows, of the cut rows, the cut
    rows' pi and pi0 in list order), and the nodes' (id, cut list)."""
    L, U, V, D = t.peek_open(N)
    ids, ncut, lists, codes = t.peek_cuts(N)
    assert len(D) == len(ids) == N
    flat = np.concatenate([lists[k, :ncut[k]] for k in range(N)] + [np.zeros(0, np.int32)])
    pi, pi0 = t.cut_rows(flat)
    out, at = [], 0
    for k in range(N):
        nc = int(ncut[k])
        out.append((D[k].tobytes(), L[k].tobytes(), U[k].tobytes(), V[k].tobytes(), codes[k, :nc].tobytes(),
                    pi[at:at + nc].tobytes(), pi0[at:at + nc].tobytes()))
        at += nc
    return out, [(int(ids[k]), lists[k, :ncut[k]].tolist()) for k in range(N)]


def step_outcome(t, MB):
    """One traced step over the whole queue: the multiset of (status, objective bits, trace_cuts row)."""
    t.set_trace(True)
    t.solve(mip_gap=0.0, frontier_batch=MB, max_steps=1)
    tr, tc = t.trace(), t.trace_cuts()
    assert len(tr['node_id']) == len(tc) > 0
    return sorted((int(s), o.tobytes(), row.tobytes()) for s, o, row in zip(tr['status'], tr['objective'], tc))


@pytest.mark.parametrize('transport', ['rccl', 'custom'])
@pytest.mark.parametrize('n,m,seed,target,MB', [(64, 32, 5, 300, 512), (256, 128, 1, 200, 512)])
def test_round_trip_is_bit_exact(n, m, seed, target, MB, transport):
    ctx = _ffi.default_context()
    comm = one_rank_comm(ctx, transport)
    prob, ints, l, u, mac = instance(ctx, n, m, seed)
    ref = grown_tree(prob, ints, l, u, mac, target, MB)
    t = grown_tree(prob, ints, l, u, mac, target, MB)
    N = t.stats()['open_nodes']
    assert ref.stats()['open_nodes'] == N <= MB
    rows = 1 << 14
    t.set_cut_migration(rows)
    t.keep_shard(0, 1)
    t.set_comm(comm, 3)
    before, lists0 = open_nodes(t, N)
    assert sorted(before) == sorted(open_nodes(ref, N)[0])
    assert any(len(li) > 0 for _, li in lists0)                     # open nodes do carry cut rows
    last_id = max(i for i, _ in lists0)
    own = len(t.cut_store()[1])

    moved = t.migrate_self(10 ** 6)                                 # every second node of the whole queue
    assert moved == min(4096, N // 2)
    after, lists1 = open_nodes(t, N)
    assert t.stats()['open_nodes'] == N
    assert sorted(after) == sorted(before)                          # the same records, bit for bit
    # the region grew by exactly the distinct store rows of the nodes that moved
    by_key = {key: li for key, (_, li) in zip(before, lists0)}
    arrived = [(key, li) for key, (i, li) in zip(after, lists1) if i > last_id]
    assert len(arrived) == moved
    distinct = set()
    for key, li in arrived:
        distinct.update(by_key[key])
    used = len(distinct)
    assert used > 0
    for key, li in arrived:
        assert all(STORE - rows <= j < STORE - rows + used for j in li)
    st = t.cut_migration_stats()
    assert st == dict(nodes_sent_with_cuts=sum(1 for _, li in arrived if li), cut_rows_sent=used,
                      cut_rows_received=used, region_rows_used=used)
    assert len(t.cut_store()[1]) == own                             # cut_store: the tree's own appends only
    g = t.global_stats()
    assert g['nodes_sent'] == g['nodes_received'] == moved
    t.set_comm(None)

    # one step over every open node: the moved tree evaluates them exactly as the one that moved nothing
    assert step_outcome(t, MB) == step_outcome(ref, MB)
    t.close(); ref.close(); prob.close()
    comm.close()


def test_option_checks():
    ctx = _ffi.default_context()
    comm = one_rank_comm(ctx, 'custom')
    prob, ints, l, u, mac = instance(ctx, 64, 32, 5)
    # no cut rounds
    plain = _ffi.Tree(prob, ints, l, u, branch_rule='pseudo cost', max_batch=64)
    with pytest.raises(_ffi.MipxError, match='no cut rounds'):
        plain.set_cut_migration(16)
    plain.close()
    S = 4096
    t = grown_tree(prob, ints, l, u, mac, 100, 64, store_capacity=S)
    with pytest.raises(_ffi.MipxError, match='must leave rows'):
        t.set_cut_migration(S)
    with pytest.raises(_ffi.MipxError, match='negative'):
        t.set_cut_migration(-1)
    own = len(t.cut_store()[1])
    assert own > 0
    with pytest.raises(_ffi.MipxError, match='more than store_capacity - rows'):
        t.set_cut_migration(S - own + 1)
    t.set_cut_migration(S - own)     # exactly what is left is fine, and it can be turned off again
    t.set_cut_migration(0)
    # off: migrate_self still refuses cut rounds
    t.keep_shard(0, 1)
    t.set_comm(comm, 3)
    with pytest.raises(_ffi.MipxError, match='without cut migration'):
        t.migrate_self(4)
    t.set_comm(None)
    # not while a step is in flight (a step hook runs with steps queued)
    seen = []

    def hook():
        try:
            t.set_cut_migration(8)
            seen.append('accepted')
        except _ffi.MipxError as e:
            seen.append(str(e))
    t.set_step_hook(hook, 1)
    t.solve(mip_gap=0.0, frontier_batch=64, max_steps=2)
    t.set_step_hook(None)
    assert seen and all('in flight' in s for s in seen), seen
    t.close()
    prob.close()
    comm.close()


def test_own_cuts_stop_at_the_lowered_cap():
    ctx = _ffi.default_context()
    prob, ints, l, u, mac = instance(ctx, 64, 32, 5)
    S, R = 1024, 1024 - 16

    def run(rows):
        t = _ffi.Tree(prob, ints, l, u, branch_rule='pseudo cost', max_batch=64, pool_capacity=1 << 15,
                      cut_params=dict(max_abs_coef=mac, store_capacity=S))
        if rows:
            t.set_cut_migration(rows)
        st = t.stats()
        while st['open_nodes'] < 300:
            st = t.solve(mip_gap=0.0, frontier_batch=64, max_steps=1)
        out = (len(t.cut_store()[1]), t.cut_stats()['dropped'])
        t.close()
        return out
    free_own, free_dropped = run(0)
    assert free_own > S - R, 'the instance must append more cuts than the lowered cap'
    own, dropped = run(R)
    assert own == S - R and dropped > free_dropped
    prob.close()


def test_table_too_small_keeps_the_nodes():
    ctx = _ffi.default_context()
    comm = one_rank_comm(ctx, 'custom')
    prob, ints, l, u, mac = instance(ctx, 64, 32, 5)
    t = grown_tree(prob, ints, l, u, mac, 300, 512)
    N = t.stats()['open_nodes']
    rows = 8
    t.set_cut_migration(rows)
    t.keep_shard(0, 1)
    t.set_comm(comm, 3)
    before, lists0 = open_nodes(t, N)
    wanted = sum(1 for _, li in lists0 if li)
    assert wanted > 0
    first = t.migrate_self(10 ** 6)
    assert 0 < first < min(4096, N // 2)            # some candidates were kept: their rows did not fit
    assert t.cut_migration_stats()['nodes_sent_with_cuts'] < wanted
    total = first
    for _ in range(3):   # the region fills up; then donations move nodes without cut rows only
        after, _ = open_nodes(t, N)
        assert t.stats()['open_nodes'] == N and sorted(after) == sorted(before)   # nothing lost
        total += t.migrate_self(10 ** 6)
    after, _ = open_nodes(t, N)
    assert t.stats()['open_nodes'] == N and sorted(after) == sorted(before)
    st = t.cut_migration_stats()
    assert 0 < st['region_rows_used'] <= rows and st['cut_rows_received'] == st['region_rows_used']
    g = t.global_stats()
    assert g['nodes_sent'] == g['nodes_received'] == total
    # the region is in use: it cannot change any more
    with pytest.raises(_ffi.MipxError, match='holds migrated cut rows'):
        t.set_cut_migration(0)
    t.set_comm(None)
    t.close()
    prob.close()
    comm.close()
