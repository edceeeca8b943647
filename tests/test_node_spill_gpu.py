"""Host spill of the frontier engine (include/mipx_spill.h).

Format: the pack kernel's records are byte-equal to a numpy encoder of the documented layout, and unpack
returns the rows bit for bit.  Engine: a run with a pool too small for the search and the spill on evaluates
the same nodes in the same order, with bit-identical results, as a run whose pool never fills."""
import numpy as np
import pytest

from simple_mip_solver_amd import BranchAndBound, MILPInstance, PseudoCostBranchNode, _ffi
from simple_mip_solver_amd.generators import random_dense_milp_arrays
from tests.support.node_rows_reference import encode, random_rows

pytestmark = pytest.mark.gpu
INF = np.inf
BIG_POOL = 1 << 20


# ---------------------------------------------------------------------------------------------- format
def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float64:
        a, b = a.view(np.uint64), b.view(np.uint64)
    return a.shape == b.shape and np.array_equal(a, b)


# counts past 1024: spill_scan gives a thread more than one record; n past 256: more than four trips of a wave
@pytest.mark.parametrize('n,nv,count', [(1, 2, 5), (7, 12, 33), (64, 65, 9), (130, 195, 70), (256, 384, 17), (63, 64, 3),
                                        (65, 67, 4), (129, 200, 1), (1024, 2047, 5), (3, 5, 1023), (3, 5, 1024), (3, 5, 1025),
                                        (2, 4, 2049), (5, 9, 4100)])
def test_pack_is_the_documented_format_and_unpack_inverts_it(n, nv, count, gpu_ctx):
    rng = np.random.default_rng(n * 1000 + nv)
    root_l, root_u, l, u, v = random_rows(rng, count, n, nv)
    off, recs = _ffi.node_pack_batch(gpu_ctx, root_l, root_u, l, u, v)
    ref_off, ref = encode(root_l, root_u, l, u, v)
    assert same_bits(off, ref_off)
    assert recs.tobytes() == ref.tobytes()
    l2, u2, v2 = _ffi.node_unpack_batch(gpu_ctx, root_l, root_u, off, recs, nv)
    assert same_bits(l2, l) and same_bits(u2, u) and same_bits(v2, v)


def cut_mode_round_trip(ctx, kcut, n, count):
    rng = np.random.default_rng(kcut)
    nv = n + 20 + kcut
    root_l, root_u, l, u, v = random_rows(rng, count, n, nv)
    ncut = rng.integers(0, kcut + 1, count).astype(np.int32)
    ncut[0], ncut[min(1, count - 1)] = 0, kcut
    ids = rng.integers(0, 1 << 20, (count, kcut)).astype(np.int32)
    off, recs = _ffi.node_pack_batch(ctx, root_l, root_u, l, u, v, ncut, ids)
    ref_off, ref = encode(root_l, root_u, l, u, v, ncut, ids)
    assert same_bits(off, ref_off) and recs.tobytes() == ref.tobytes()
    seed = np.full((count, kcut), -7, np.int32)
    l2, u2, v2, nc2, ids2 = _ffi.node_unpack_batch(ctx, root_l, root_u, off, recs, nv, kcut=kcut, cut_ids=seed)
    assert same_bits(l2, l) and same_bits(u2, u) and same_bits(v2, v) and same_bits(nc2, ncut)
    for k in range(count):   # the record's ids; beyond ncut what the caller's buffer held
        assert same_bits(ids2[k, :ncut[k]], ids[k, :ncut[k]])
        assert np.all(ids2[k, ncut[k]:] == -7)


@pytest.mark.parametrize('kcut', [1, 5, 64])
def test_pack_and_unpack_in_cut_mode(kcut, gpu_ctx):
    cut_mode_round_trip(gpu_ctx, kcut, 40, 25)


@pytest.mark.parametrize('kcut,n,count', [(63, 65, 5), (64, 129, 3), (2, 3, 1025), (3, 2, 4100)])
def test_pack_and_unpack_in_cut_mode_at_other_widths_and_counts(kcut, n, count, gpu_ctx):
    cut_mode_round_trip(gpu_ctx, kcut, n, count)


def test_pack_reports_the_room_it_needs(gpu_ctx):
    rng = np.random.default_rng(3)
    root_l, root_u, l, u, v = random_rows(rng, 6, 10, 15)
    L = _ffi.lib()
    off = np.zeros(7, np.int64)
    used = np.zeros(1, np.int64)
    small = np.zeros(8, np.uint8)
    rc = L.mipx_node_pack_batch(gpu_ctx._h, 10, 15, 6, _ffi._ptr(root_l), _ffi._ptr(root_u), _ffi._ptr(l),
                                _ffi._ptr(u), _ffi._ptr(v), None, None, 0, _ffi._ptr(off), _ffi._ptr(small), 8,
                                _ffi._ptr(used))
    assert rc == -5   # MIPX_ENOMEM
    assert used[0] == encode(root_l, root_u, l, u, v)[0][-1]


# ---------------------------------------------------------------------------------------------- engine
def headroom(batch, dive):
    return (3 if batch > 1 else 1) * batch * (2 * (1 + dive) + 1)


def min_pool(batch, dive):
    return 2 * headroom(batch, dive) + 1


CUTS = dict(max_abs_coef=1e4, exact_tableau=1)


def run(ctx, inst, rule, search, batch, dive, pool, spill=None, trace=False, cuts=False):
    A, b, c, l, u, ints = inst
    p = _ffi.Problem(ctx, A, b, c)
    t = _ffi.Tree(p, ints, l, u, branch_rule=rule, search_rule=search, max_batch=batch, pool_capacity=pool,
                  cut_params=CUTS if cuts else None)
    if batch > 1 and not cuts:
        t.set_anchor_mode(True)
        t.set_dive(dive)
    if trace:
        t.set_trace(True)
    if spill:
        t.set_host_spill(spill)
    st = t.solve(mip_gap=1e-9, max_seconds=120.0)
    out = dict(st=st, spill=t.spill_stats(), pc=t.pseudo_cost_arrays(),
               x=t.solution() if st['has_solution'] else None, trace=t.trace() if trace else None)
    t.close()
    p.close()
    return out


# rule, search, frontier batch, dive, cut rounds, traced comparison.  Pseudo costs with batches of 64 are compared
# on the device finish only: their host-finished (traced) pipeline is not reproducible from run to run even with
# a pool that never fills (the trace of two such runs can part after 10^4 nodes), so it cannot be the yardstick.
CASES = [
    ('most fractional', 'best first', 1, 0, False, True),
    ('pseudo cost', 'best first', 1, 0, False, True),
    ('most fractional', 'depth first', 1, 0, False, True),
    ('most fractional', 'depth first', 64, 0, False, True),
    ('most fractional', 'best first', 64, 0, False, True),
    ('most fractional', 'best first', 64, 4, False, True),
    ('pseudo cost', 'best first', 64, 0, False, False),
    ('pseudo cost', 'best first', 64, 4, False, False),
    ('pseudo cost', 'best first', 4, 0, True, True),
]
SIZES = [(30, 15), (40, 20), (60, 30), (80, 40)]
_found = {}


def exhausting_instance(ctx, rule, search, batch, dive, cuts):
    """The first small random instance whose search does not fit into the smallest pool the spill accepts
    (the run without the spill ends with pool_exhausted) and whose spill run reloads nodes (spilled nodes are
    not always popped again: the incumbent may close them first)."""
    key = (rule, search, batch, dive, cuts)
    if key not in _found:
        pool = min_pool(batch, dive)
        _found[key] = None
        for n, m in SIZES:
            for seed in range(3):
                inst = random_dense_milp_arrays(n, m, seed=seed)
                r = run(ctx, inst, rule, search, batch, dive, pool, cuts=cuts)
                if r['st']['pool_exhausted']:
                    assert r['st']['status'] == 4
                    if run(ctx, inst, rule, search, batch, dive, pool, spill=1 << 30, cuts=cuts)['spill']['reloaded'] > 0:
                        _found[key] = (inst, pool)
                        break
            if _found[key] is not None:
                break
    assert _found[key] is not None, f'no instance of {SIZES} fills a pool of {min_pool(batch, dive)} rows'
    return _found[key]


def assert_same_end(a, b):
    sa, sb = a['st'], b['st']
    for k in ('status', 'evaluated_nodes', 'lp_solved', 'probes_solved', 'pivots', 'created_nodes', 'steps', 'dives',
              'has_solution'):
        assert sa[k] == sb[k], (k, sa[k], sb[k])
    for k in ('primal_bound', 'dual_bound', 'gap'):
        assert same_bits(np.float64(sa[k]), np.float64(sb[k])), (k, sa[k], sb[k])
    assert (a['x'] is None) == (b['x'] is None)
    if a['x'] is not None:
        assert same_bits(a['x'], b['x'])
    for pa, pb in zip(a['pc'], b['pc']):
        assert same_bits(pa, pb)


@pytest.mark.parametrize('rule,search,batch,dive,cuts,traced', CASES)
def test_spill_run_is_the_big_pool_run(rule, search, batch, dive, cuts, traced, gpu_ctx):
    inst, pool = exhausting_instance(gpu_ctx, rule, search, batch, dive, cuts)
    for trace in (True, False)[0 if traced else 1:]:   # traced: the host finish; untraced: the device finish where it applies
        big = run(gpu_ctx, inst, rule, search, batch, dive, BIG_POOL, trace=trace, cuts=cuts)
        spl = run(gpu_ctx, inst, rule, search, batch, dive, pool, spill=1 << 30, trace=trace, cuts=cuts)
        assert big['st']['status'] == 1 and not big['st']['pool_exhausted']
        assert spl['st']['status'] == 1 and not spl['st']['pool_exhausted']
        s = spl['spill']
        assert s['spilled'] > 0 and s['reloaded'] > 0 and s['events'] > 0 and s['peak_host_bytes'] > 0
        # the records one spill event moved: at least the mean, at most the pool's rows and the run's total
        print(f'spill events [{rule}, {search}, batch {batch}, dive {dive}, cuts {cuts}, traced {trace}]: pool {pool}, '
              f'{s["spilled"]} records in {s["events"]} events, largest event between {-(-s["spilled"] // s["events"])} and '
              f'{min(s["spilled"], pool)}')
        assert 0 <= s['on_host'] <= s['spilled'] - s['reloaded']   # (the rest closed unevaluated: dropped)
        assert big['spill']['spilled'] == 0
        if trace:
            for k in ('node_id', 'status', 'branch_var', 'objective'):
                assert same_bits(spl['trace'][k], big['trace'][k]), k
        assert_same_end(spl, big)


def test_peek_open_after_spilling_matches_the_big_pool(gpu_ctx):
    rule, search, batch, dive = 'most fractional', 'best first', 1, 0
    (A, b, c, l, u, ints), pool = exhausting_instance(gpu_ctx, rule, search, batch, dive, False)
    p = _ffi.Problem(gpu_ctx, A, b, c)
    trees = [_ffi.Tree(p, ints, l, u, branch_rule=rule, max_batch=1, pool_capacity=cap) for cap in (pool, BIG_POOL)]
    trees[0].set_host_spill(1 << 30)
    calls = 0
    while True:
        st = [t.solve(mip_gap=1e-9, max_steps=1) for t in trees]
        calls += 1
        assert st[0]['status'] == 4 and st[1]['status'] == 4, 'the search ended before a node was spilled'
        if trees[0].spill_stats()['on_host'] > 2:
            break
    assert st[0]['open_nodes'] == st[1]['open_nodes']
    k = st[0]['open_nodes']
    got = []
    for t in trees:
        ids = t.peek_cuts(k)[0]
        got.append((ids,) + tuple(t.peek_open(k)))
    for a, b2 in zip(got[0], got[1]):
        assert same_bits(a, b2)
    for t in trees:
        t.close()
    p.close()


def test_host_cap_too_small_stops_like_a_full_pool(gpu_ctx):
    rule, search, batch, dive = 'most fractional', 'best first', 1, 0
    inst, pool = exhausting_instance(gpu_ctx, rule, search, batch, dive, False)
    r = run(gpu_ctx, inst, rule, search, batch, dive, pool, spill=64)
    assert r['st']['status'] == 4 and r['st']['pool_exhausted'] == 1
    assert r['spill']['spilled'] == 0


def test_invalid_spill_arguments(gpu_ctx):
    A, b, c, l, u, ints = random_dense_milp_arrays(20, 10, seed=0)
    p = _ffi.Problem(gpu_ctx, A, b, c)
    t = _ffi.Tree(p, ints, l, u, max_batch=64, pool_capacity=min_pool(64, 0) - 1)
    with pytest.raises(_ffi.MipxError):   # pool below the headroom
        t.set_host_spill(1 << 20)
    t.close()
    t = _ffi.Tree(p, ints, l, u, max_batch=64, pool_capacity=min_pool(64, 0))
    t.set_host_spill(1 << 20)
    t.set_dive(4)   # the headroom grows past the pool: solve refuses
    with pytest.raises(_ffi.MipxError):
        t.solve(frontier_batch=64)
    t.close()
    comm = _ffi.Comm(gpu_ctx, 0, 1, allgather=lambda x: [x], send=lambda q, d: None, recv=lambda q, k: b'')
    t = _ffi.Tree(p, ints, l, u, max_batch=4, pool_capacity=1 << 12)
    t.set_comm(comm)
    with pytest.raises(_ffi.MipxError):   # not with a communicator ...
        t.set_host_spill(1 << 20)
    t.close()
    t = _ffi.Tree(p, ints, l, u, max_batch=4, pool_capacity=1 << 12)
    t.set_host_spill(1 << 20)
    with pytest.raises(_ffi.MipxError):   # ... either way round
        t.set_comm(comm)
    t.close()
    comm.close()
    p.close()


# ---------------------------------------------------------------------------------------------- Python surface
def test_branch_and_bound_with_host_spill(gpu_ctx):
    from scipy.optimize import Bounds, LinearConstraint, milp
    import warnings
    (A, b, c, l, u, ints), pool = exhausting_instance(gpu_ctx, 'pseudo cost', 'best first', 64, 4, False)

    def model():
        return MILPInstance(A=A, b=b, c=c, l=l, u=u, sense=['Min', '>='], integerIndices=ints, numVars=len(c))
    big = BranchAndBound(model(), Node=PseudoCostBranchNode, pseudo_costs={}, gomory_cuts=False,
                         frontier_batch=64, dive=4, pool_capacity=BIG_POOL)
    big.solve()
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        bb = BranchAndBound(model(), Node=PseudoCostBranchNode, pseudo_costs={}, gomory_cuts=False,
                            frontier_batch=64, dive=4, pool_capacity=pool, host_spill=True)
        bb.solve()
    assert bb.status == big.status == 'optimal'
    assert bb.objective_value == big.objective_value
    assert bb.evaluated_nodes == big.evaluated_nodes
    assert bb.spill_stats['spilled'] > 0 and bb.spill_stats['reloaded'] > 0
    integrality = np.zeros(len(c))
    integrality[ints] = 1
    h = milp(c, constraints=LinearConstraint(A, lb=b, ub=np.inf), bounds=Bounds(l, u), integrality=integrality,
             options={'mip_rel_gap': 0.0, 'time_limit': 120})
    assert h.status == 0
    assert abs(bb.objective_value - h.fun) <= 1e-6 * max(1.0, abs(h.fun))
    with pytest.warns(RuntimeWarning, match='host spill store'):
        small = BranchAndBound(model(), Node=PseudoCostBranchNode, pseudo_costs={}, gomory_cuts=False,
                               frontier_batch=64, dive=4, pool_capacity=pool, host_spill=64)
        small.solve()
    assert small.status != 'optimal' and small.evaluated_nodes < big.evaluated_nodes


# ---------------------------------------------------------------------------------------------- spill turned off, reanchor
def stepwise(ctx, inst, rule, batch, dive, pool, spill, until_on_host, then):
    """Solve in single steps until `until_on_host` nodes are on the host (or, for the big pool, as many calls as the
    other tree made: `until_on_host` is then the call count), apply `then(tree, stats)`, solve to the end traced."""
    A, b, c, l, u, ints = inst
    p = _ffi.Problem(ctx, A, b, c)
    t = _ffi.Tree(p, ints, l, u, branch_rule=rule, max_batch=batch, pool_capacity=pool)
    if batch > 1:
        t.set_anchor_mode(True)
        t.set_dive(dive)
    t.set_trace(True)
    if spill:
        t.set_host_spill(spill)
    calls = 0
    while True:
        st = t.solve(mip_gap=1e-9, frontier_batch=batch, max_steps=1)
        calls += 1
        assert st['status'] == 4 and not st['pool_exhausted'], 'the search ended before the checkpoint'
        if (spill and t.spill_stats()['on_host'] >= until_on_host) or (not spill and calls == until_on_host):
            break
    then(t, st)
    st = t.solve(mip_gap=1e-9, max_seconds=120.0)
    out = dict(st=st, calls=calls, trace=t.trace(), spill=t.spill_stats(), x=t.solution() if st['has_solution'] else None,
               pc=t.pseudo_cost_arrays())
    t.close()
    p.close()
    return out


def test_reanchor_after_spilling_gives_the_big_pool_anchors(gpu_ctx):
    """mipx_tree_reanchor decodes the spilled nodes for its refactor launch: after re-anchoring every open node of a
    spilled tree, the search goes on exactly as the one of a pool that never filled."""
    rule, batch, dive = 'most fractional', 64, 0
    inst, pool = exhausting_instance(gpu_ctx, rule, 'best first', batch, dive, False)
    reanchor = lambda t, st: t.reanchor(st['open_nodes'])   # noqa: E731
    spl = stepwise(gpu_ctx, inst, rule, batch, dive, pool, 1 << 30, 8, reanchor)
    big = stepwise(gpu_ctx, inst, rule, batch, dive, BIG_POOL, None, spl['calls'], reanchor)
    assert spl['st']['status'] == 1 and spl['spill']['spilled'] > 0
    for k in ('node_id', 'status', 'branch_var', 'objective'):
        assert same_bits(spl['trace'][k], big['trace'][k]), k
    assert_same_end(spl, big)


@pytest.mark.parametrize('batch,dive', [(1, 0), (64, 0)])
def test_turning_the_spill_off_with_nodes_on_the_host(batch, dive, gpu_ctx):
    """Spill for a while, turn the spill off, solve on in the tight pool: the nodes on the host still come back,
    the batches leave rows for them, and the search either finishes or stops on the full pool -- never an error."""
    rule = 'most fractional'
    inst, pool = exhausting_instance(gpu_ctx, rule, 'best first', batch, dive, False)
    r = stepwise(gpu_ctx, inst, rule, batch, dive, pool, 1 << 30, 4, lambda t, st: t.set_host_spill(0))
    s = r['spill']
    assert r['st']['status'] in (1, 4)
    assert r['st']['status'] == 1 or r['st']['pool_exhausted'] == 1
    assert s['spilled'] > 0 and 0 <= s['on_host'] <= s['spilled'] - s['reloaded']
    if r['st']['status'] == 1 and batch == 1:   # it finished one node per step: the same search as the big pool's
        big = run(gpu_ctx, inst, rule, 'best first', batch, dive, BIG_POOL, trace=True)
        assert same_bits(r['trace']['node_id'], big['trace']['node_id'])
