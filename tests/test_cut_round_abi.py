"""The kernels of a cut round on a caller's data (include/mipx_cutround.h), the parts that need no GPU: the header
against the ctypes table and the exported symbols, that the engine and the scaffolding launch the kernels from one
place, and the restatement the kernels are compared with (tests/support/cut_round_reference.py): hand-worked rounds, its
invariants on every case, and that the cases reach every path the GPU test is there for."""
import collections
import os

import numpy as np
import pytest

from simple_mip_solver_amd import _ffi
from tests.support import cut_round_reference as ref
from tests.support.abi_check import agrees, library_prerequisites, prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ['mipx_cut_round_begin_batch', 'mipx_cut_round_generate_batch']
F = ref.F


def test_header_and_signature_table_agree():
    protos = prototypes('mipx_cutround.h')
    assert sorted(protos) == sorted(_ffi.CUTROUND_SYMBOLS) == sorted(NAMES)
    for name, (ret, params) in protos.items():
        restype, argtypes = _ffi._CUTROUND_SIGNATURES[name]
        assert agrees(ret, restype), name
        assert len(params) == len(argtypes), name
        for k, (decl, ctype) in enumerate(zip(params, argtypes)):
            assert agrees(decl, ctype), f'{name} parameter {k} is `{decl}`, the table says {ctype}'
    assert _ffi.CUT_FIELDS == ref.FIELDS


def test_new_symbols_overlap_no_existing_list():
    old = set()
    for attr in dir(_ffi):
        if attr.endswith('SYMBOLS') and attr != 'CUTROUND_SYMBOLS':
            old |= set(getattr(_ffi, attr))
    assert old and not set(_ffi.CUTROUND_SYMBOLS) & old


def test_mipx_h_includes_the_header_and_keeps_its_version():
    text = open(os.path.join(ROOT, 'include', 'mipx.h')).read()
    assert '#include "mipx_cutround.h"' in text
    assert _ffi.lib().mipx_abi_version() == 1
    assert 'TEST SCAFFOLDING' in open(os.path.join(ROOT, 'include', 'mipx_cutround.h')).read()


def test_library_exports_the_entries():
    L = _ffi.lib()
    for name in _ffi.CUTROUND_SYMBOLS:
        assert hasattr(L, name), name
        assert getattr(L, name).restype is _ffi._CUTROUND_SIGNATURES[name][0]


def test_c_entries_refuse_null_arguments():
    L = _ffi.lib()
    assert L.mipx_cut_round_begin_batch(None, 5, 3, 8, 1, 0, 5, 1e-4, 1e9, 1, 0, 0, *([None] * 16)) == -1      # MIPX_EINVAL
    assert L.mipx_cut_round_generate_batch(None, 1, 8, 16, 0, 0, 10, 1e3, 5, 1e-8, 0.98, 1e6, *([None] * 22)) == -1


def test_no_product_code_calls_the_scaffolding():
    pkg = os.path.join(ROOT, 'simple_mip_solver_amd')
    for base, _, files in os.walk(pkg):
        for f in files:
            if f.endswith('.py') and f != '_ffi.py':
                text = open(os.path.join(base, f)).read()
                assert 'cut_round_begin_batch' not in text and 'cut_round_generate_batch' not in text, f


def test_the_round_kernels_are_launched_from_one_place():
    """The engine's form of the six launches stands once, in enqueue_cut_begin and enqueue_cut_generate of
    tree_engine.hip.h; the engine and cutround_api.hip.h both go through them.  (mipx.hip keeps the stand-alone K2 and K3
    of mipx_gomory_batch and mipx_cut_select_batch.)"""
    csrc = os.path.join(ROOT, 'simple_mip_solver_amd', 'csrc')
    kernels = ('cut_gather_state', 'cut_round_begin', 'pool_append', 'cut_round_apply', 'gomory_cuts<', 'select_cuts')
    hits = [(f, line.strip()) for f in sorted(os.listdir(csrc)) if f.endswith(('.h', '.hip'))
            for line in open(os.path.join(csrc, f)) if 'hipLaunchKernelGGL' in line and any(k in line for k in kernels)]
    engine = [line for f, line in hits if f == 'tree_engine.hip.h']
    assert {f for f, _ in hits} <= {'tree_engine.hip.h', 'mipx.hip'}
    assert all(sum(k in line for line in engine) == 1 for k in kernels), engine
    assert not any(k in line for f, line in hits if f == 'mipx.hip' for k in kernels[:4])
    text = open(os.path.join(csrc, 'tree_engine.hip.h')).read()
    api = open(os.path.join(csrc, 'cutround_api.hip.h')).read()
    assert text.count('enqueue_cut_begin(') == 3 and text.count('enqueue_cut_generate(') == 2          # the definition and the engine's calls
    assert api.count('enqueue_cut_begin(') == 1 and api.count('enqueue_cut_generate(') == 1 and 'hipLaunchKernelGGL' not in api
    assert text.rstrip().endswith('#include "cutround_api.hip.h"')
    assert os.path.join(ROOT, 'include', 'mipx_cutround.h') in library_prerequisites()   # (a change of the header rebuilds the library)


# ---- hand-worked rounds ------------------------------------------------------------------------------------------
def tiny_begin(**over):
    """n = 2, m0 = 1, kc = 4, three nodes with lists (10, 11, 12), (20,), () and basis codes 1..7 per node."""
    B, n, m0, kc = 3, 2, 1, 4
    s = dict(n=n, m0=m0, kc=kc, B=B, round=0, max_rounds=3, progress_tol=1e-4, max_dual_bound=50.0, have_dump=1, gather=0,
             status=np.array([0, 0, 0], np.int32), obj=np.array([5.0, 6.0, 7.0]), mipf=np.zeros(B, np.int32),
             y=np.array([[1.0, 0.5, 0.0, -2.0, 9.0], [1.0, 0.25, 9.0, 9.0, 9.0], [1.0, 9.0, 9.0, 9.0, 9.0]]),
             vstat=np.tile(np.arange(1, 8, dtype=np.int8), (B, 1)), ncut=np.array([3, 1, 0], np.int32),
             ids=np.array([[10, 11, 12, 99], [20, 99, 99, 99], [99, 99, 99, 99]], np.int32),
             state=np.zeros((len(ref.FIELDS), B), np.int32), obj_before=np.array([1.0, 2.0, 3.0]), active=np.full(B, 7, np.int32),
             counters=np.array([0, 40, 41, 0], np.int32))
    s.update(over)
    return s


def test_hand_worked_begin_removes_the_slack_cut_and_keeps_the_tail():
    w = ref.begin(tiny_begin())
    # node 0: the dual of its second cut row is 0 -> ids (10, 12), the codes of rows 1 and 3 move up; the third entries stay
    assert w['ncut'].tolist() == [2, 1, 0]
    assert w['ids'].tolist() == [[10, 12, 12, 99], [20, 99, 99, 99], [99, 99, 99, 99]]
    assert w['vstat'][0].tolist() == [1, 2, 3, 4, 6, 6, 7] and w['vstat'][1].tolist() == [1, 2, 3, 4, 5, 6, 7]
    assert w['active'].tolist() == [1, 1, 1] and w['resolve'].tolist() == [1, 0, 0] and w['need_tab'].tolist() == [1, 0, 0]
    assert w['state'][F['rounds']].tolist() == [1, 1, 1] and w['state'][F['it_removed']].tolist() == [1, 0, 0]
    assert w['state'][F['n_removed']].tolist() == [1, 0, 0] and w['obj_before'].tolist() == [5.0, 6.0, 7.0]
    assert w['counters'].tolist() == [3, 40, 41, 1]
    assert w['paths']['remove_mixed'] == 1 and w['paths']['remove_none'] == 1 and w['paths']['tableau_after_removal'] == 1
    # without a dumped tableau every generating node needs one
    assert ref.begin(tiny_begin(have_dump=0))['need_tab'].tolist() == [1, 1, 1]


def test_hand_worked_begin_stall_test_and_loop_condition():
    state = np.zeros((len(ref.FIELDS), 3), np.int32)
    state[F['rounds']] = (1, 3, 1)
    # round 1: node 0 moved from 5 to 5.0004 (8e-5 of 5: stalled); node 1 has had its three rounds; node 2 was not
    # generating in the round before (it is not tested although 7 == 7), and its objective is at the bound
    w = ref.begin(tiny_begin(round=1, obj=np.array([5.0004, 9.0, 7.0]), obj_before=np.array([5.0, 6.0, 7.0]), state=state,
                             active=np.array([1, 1, 0], np.int32), max_dual_bound=7.0))
    assert w['state'][F['stalled']].tolist() == [1, 0, 0] and w['active'].tolist() == [0, 0, 0]
    assert w['ncut'].tolist() == [3, 1, 0] and w['state'][F['rounds']].tolist() == [1, 3, 1]       # nothing is removed or counted
    assert w['resolve'].tolist() == [0, 0, 0] and w['need_tab'].tolist() == [0, 0, 0] and w['counters'].tolist() == [0, 40, 41, 0]
    assert w['obj_before'].tolist() == [5.0, 6.0, 7.0]
    assert w['paths']['stalls_now'] == 1 and w['paths']['rounds_at_max'] == 1 and w['paths']['obj_at_bound'] == 1 and w['paths']['was_inactive'] == 1
    # 0 / 0 and x / 0 do not stall; an infeasible LP stops the node whatever its objective holds
    w = ref.begin(tiny_begin(round=1, obj=np.array([0.0, 4.0, np.nan]), obj_before=np.zeros(3), status=np.array([0, 2, 1], np.int32),
                             active=np.ones(3, np.int32)))
    assert w['state'][F['stalled']].tolist() == [0, 0, 0] and w['active'].tolist() == [1, 1, 0]


def test_hand_worked_gather():
    s = tiny_begin(gather=1, slot=np.array([4, 0, 2], np.int32), pool_ncut=np.array([1, 4, 0, 4, 2], np.int32),
                   pool_ids=np.arange(20, dtype=np.int32).reshape(5, 4), state=np.full((len(ref.FIELDS), 3), 8, np.int32))
    g = ref.gather(s)
    assert g['ncut'].tolist() == [2, 1, 0] and g['ids'].tolist() == [[16, 17, 12, 99], [0, 99, 99, 99], [99, 99, 99, 99]]
    assert not g['state'].any() and g['counters'].tolist() == [0, 40, 41, 0]
    s['counters'][2] = 1
    assert ref.gather(s)['counters'].tolist() == [0, 40, 2, 0]


class PlantedOracle:
    """An oracle whose K2 makes the cuts a test plants; the selection is the real one (it needs no GPU)."""

    def __init__(self, cuts):
        self.cuts = cuts

    def gomory_from_dump(self, A, b, dump, x, int_idx, max_term):
        return dict(safe_pi=np.array([c[0] for c in self.cuts], np.float64).reshape(len(self.cuts), A.shape[1]),
                    safe_pi0=np.array([c[1] for c in self.cuts], np.float64))

    def select_cuts(self, *args):
        from oracle import oracle
        return oracle.select_cuts(*args)


def tiny_generate(**over):
    """n = 3, m = 2, kc = 2, one node without cut rows whose basis (x0, x1) gives two cuts at x = (0.5, 0.5, 0);
    slab of 4 rows, 2 taken (row 0 left the pool earlier, row 1: x2 >= 1 is in it), a store of 6 with 4 used."""
    n, m, kc = 3, 2, 2
    s = dict(ref.DEFAULTS, A=-np.eye(2, 3), b=-np.ones(2), is_int=np.ones(n, np.uint8), B=1, kc=kc, slab_rows=4, store_cap=6,
             max_nonzero_coefs=3, active=np.ones(1, np.int32), ncut=np.zeros(1, np.int32), ids=np.full((1, kc), 99, np.int32),
             T=np.zeros((1, m + kc, n)), idx=np.array([[2, 3, 4, 0, 1, -5, -5, 0, 0, 0]], np.int32),
             vstat=np.array([[1, 1, 3, 3, 3, 9, 9]], np.int8), x=np.array([[0.5, 0.5, 0.0]]),
             state=np.zeros((len(ref.FIELDS), 1), np.int32), pool_list=np.array([[1, -9, -9, -9]], np.int32),
             slab_pi=np.full((1, 4, n), ref.STALE_SLAB), slab_pi0=np.full((1, 4), ref.STALE_SLAB),
             store_pi=np.full((6, n), ref.STALE_STORE), store_pi0=np.full(6, ref.STALE_STORE), store_count=np.array([4], np.int32),
             resolve=np.zeros(1, np.int32), counters=np.array([1, 0, 0, 0], np.int32))
    s['slab_pi'][0, 1], s['slab_pi0'][0, 1] = (0.0, 0.0, 1.0), 1.0
    s['state'][F['slab_n'], 0], s['state'][F['pool_n'], 0] = 2, 1
    s.update(over)
    return s


CUTS = [((1.0, 0.0, 0.0), 1.0), ((0.0, 1.0, 0.0), 2.0)]         # x0 >= 1 (depth -0.5), x1 >= 2 (depth -1.5)


def test_hand_worked_pool_append_and_apply():
    w = ref.generate(tiny_generate(), PlantedOracle(CUTS))
    # pool_append: two cuts made, rows 2 and 3 of the slab, the pool (1, 2, 3)
    assert w['k2_ncuts'] == [2] and w['slab_pi'][0, 2].tolist() == [1.0, 0.0, 0.0] and w['slab_pi0'][0].tolist() == [ref.STALE_SLAB, 1.0, 1.0, 2.0]
    assert w['state'][F['slab_n'], 0] == 4 and w['state'][F['it_created'], 0] == 1 and w['state'][F['n_created'], 0] == 2
    # K3 at x = (0.5, 0.5, 0): depths -1 (x2 >= 1), -0.5, -1.5 -> pool positions 2, 0, 1 in that order, all orthogonal
    assert w['k3_added'] == [[2, 0, 1]] and w['k3_term'] == [0]
    # apply: the list has room for two, the store for two: ids 4 and 5 hold x1 >= 2 and x2 >= 1; the third is dropped; the
    # whole selection has left the pool; pool_list keeps the marks of the in-place compaction
    assert w['ncut'].tolist() == [2] and w['ids'].tolist() == [[4, 5]] and w['store_count'].tolist() == [6]
    assert w['store_pi'][4].tolist() == [0.0, 1.0, 0.0] and w['store_pi0'][4:].tolist() == [2.0, 1.0] and w['store_pi'][5].tolist() == [0.0, 0.0, 1.0]
    assert w['vstat'].tolist() == [[1, 1, 3, 3, 3, 1, 1]]
    assert w['state'][F['pool_n'], 0] == 0 and w['pool_list'].tolist() == [[-1, -1, -1, -9]]
    assert [int(w['state'][F[f], 0]) for f in ('it_added', 'n_added', 'dropped', 'ncut_out')] == [1, 3, 1, 2]
    assert w['resolve'].tolist() == [1] and w['counters'].tolist() == [1, 1, 2, 0]
    assert w['paths']['list_room_short_2'] == 1 and w['paths']['store_room_exact'] == 1 and w['paths']['selects_all'] == 1


def test_hand_worked_full_slab_and_full_store():
    # three rows of the slab taken: of the two cuts made only the first fits; it is counted as created all the same
    s = tiny_generate()
    s['state'][F['slab_n'], 0] = 3
    s['slab_pi'][0, 2], s['slab_pi0'][0, 2] = (0.0, 0.0, 5.0), -1.0             # (an old row that left the pool)
    w = ref.generate(s, PlantedOracle(CUTS))
    assert w['state'][F['slab_n'], 0] == 4 and w['state'][F['n_created'], 0] == 2 and w['slab_pi0'][0, 3] == 1.0
    assert w['k3_added'] == [[0, 1]] and w['pool_list'].tolist() == [[-1, -1, -9, -9]]     # x2 >= 1, then x0 >= 1
    assert w['state'][F['dropped'], 0] == 1 and w['ids'].tolist() == [[4, 5]] and w['paths']['slab_overflow_by_1'] == 1
    # a store with one entry left: the node asks for every cut its list still has room for -- after the first all three
    # times, since a lost entry takes no room in the list -- and the ids 6 and 7 lie past the cap
    w = ref.generate(tiny_generate(store_count=np.array([5], np.int32)), PlantedOracle(CUTS))
    assert w['store_count'].tolist() == [8] and w['ids'].tolist() == [[5, 99]] and w['ncut'].tolist() == [1]
    assert [int(w['state'][F[f], 0]) for f in ('n_added', 'dropped')] == [3, 2] and w['store_pi0'][5] == 2.0
    # a full list asks for nothing: the store count stays, everything selected is dropped, the LP did not change
    s = tiny_generate(ncut=np.array([2], np.int32), ids=np.array([[0, 1]], np.int32), vstat=np.array([[1, 1, 3, 3, 3, 1, 1]], np.int8),
                      idx=np.array([[2, 3, 4, 0, 1, 5, 6, 0, 0, 0]], np.int32))
    s['store_pi'][:2], s['store_pi0'][:2] = 0.0, 0.0
    w = ref.generate(s, PlantedOracle(CUTS))
    assert w['store_count'].tolist() == [4] and w['state'][F['dropped'], 0] == 3 and w['resolve'].tolist() == [0] and w['counters'].tolist() == [1, 0, 2, 0]
    assert w['state'][F['pool_n'], 0] == 0 and w['paths']['list_room_0'] == 1


def test_count_cuts_window():
    is_int = np.array([1, 1, 1, 0, 1], np.uint8)
    x = np.array([2.5, 3.0099, -0.5, 0.5, 7.995])
    # 2.5 counts; 3.0099 and 7.995 lie outside the window [0.01, 0.99]; -0.5 reads as 0; column 3 is continuous
    assert ref.count_cuts(5, [0, 1, 2, 3, 4, 6], x, is_int) == 1
    assert ref.count_cuts(5, [5, 6, 7], x, is_int) == 0


# ---- the restatement on every case -------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ref.BEGIN_CASES)
def test_invariants_of_begin(name):
    s, w = ref.case(name)
    B, n, m0, kc = s['B'], s['n'], s['m0'], s['kc']
    src = ref.gather(s) if s['gather'] else s
    act = w['active'] == 1
    assert set(np.unique(w['active'])) <= {0, 1} and w['counters'][0] - s['counters'][0] == act.sum()
    assert w['counters'][3] - s['counters'][3] == w['need_tab'].sum() and w['counters'][1] == s['counters'][1]
    assert np.all(w['need_tab'] >= w['resolve']) and np.all(w['resolve'] <= w['active'])
    if s['have_dump']:
        assert np.array_equal(w['need_tab'], w['resolve'])
    removed = np.asarray(src['ncut']) - w['ncut']
    assert np.all(removed >= 0) and np.all(removed[~act] == 0) and np.array_equal(w['resolve'] == 1, removed > 0)
    st0, st1 = np.asarray(src['state']), w['state']
    assert np.array_equal(st1[F['rounds']] - st0[F['rounds']], act.astype(int)) and np.array_equal(st1[F['n_removed']] - st0[F['n_removed']], removed)
    assert np.all(st1[F['stalled']] >= st0[F['stalled']]) and np.all(st1[F['rounds']] <= s['max_rounds'])
    for f in ('it_created', 'n_created', 'it_added', 'n_added', 'ncut_out', 'pool_n', 'slab_n', 'dropped'):
        assert np.array_equal(st1[F[f]], st0[F[f]]), f
    for k in range(B):
        nc0, nc1 = int(src['ncut'][k]), int(w['ncut'][k])
        # the kept ids are a subsequence of the old list, the tail is as it was
        it = iter(np.asarray(src['ids'])[k, :nc0].tolist())
        assert all(i in it for i in w['ids'][k, :nc1].tolist())
        assert np.array_equal(w['ids'][k, nc1:], np.asarray(src['ids'])[k, nc1:])
        assert np.array_equal(w['vstat'][k, :n + m0], s['vstat'][k, :n + m0]) and np.array_equal(w['vstat'][k, n + m0 + nc1:], s['vstat'][k, n + m0 + nc1:])
        if act[k]:
            assert w['obj_before'][k] == s['obj'][k] and s['status'][k] in (0, 2) and s['obj'][k] < s['max_dual_bound']
        else:
            assert w['obj_before'][k] == s['obj_before'][k]


@pytest.mark.parametrize('name', ref.GENERATE_CASES)
def test_invariants_of_generate(name):
    s, w = ref.case(name)
    B, kc, SR, cap = s['B'], s['kc'], s['slab_rows'], s['store_cap']
    st0, st1 = np.asarray(s['state']), w['state']
    count0 = int(s['store_count'][0])
    handed = []
    for k in range(B):
        p = w['per_node'][k]
        if p is None:
            assert w['k2_ncuts'][k] is None and np.array_equal(st1[:, k], st0[:, k]) and np.array_equal(w['pool_list'][k], s['pool_list'][k])
            continue
        made, nadd = w['k2_ncuts'][k], w['k3_nadded'][k]
        kept = st1[F['slab_n'], k] - st0[F['slab_n'], k]
        assert 0 <= kept <= made and st1[F['slab_n'], k] <= SR and (kept == made or st1[F['slab_n'], k] == SR)
        assert st1[F['n_created'], k] - st0[F['n_created'], k] == made and st1[F['n_added'], k] - st0[F['n_added'], k] == nadd
        assert st1[F['pool_n'], k] == st0[F['pool_n'], k] + kept - nadd
        took = int(w['ncut'][k]) - p['nc0']
        assert 0 <= took <= p['wanted'] <= kc - p['nc0'] and st1[F['ncut_out'], k] == w['ncut'][k] <= kc
        assert st1[F['dropped'], k] - st0[F['dropped'], k] == (made - kept) + (nadd - took)
        # the pool afterwards: its old and new entries in order, without the selected ones
        before = np.concatenate([s['pool_list'][k, :st0[F['pool_n'], k]], st0[F['slab_n'], k] + np.arange(kept)])
        assert np.array_equal(w['pool_list'][k, :st1[F['pool_n'], k]], np.delete(before, np.array(w['k3_added'][k], int)))
        assert len(set(w['k3_added'][k])) == nadd and all(0 <= a < len(before) for a in w['k3_added'][k])
        new = w['ids'][k, p['nc0']:w['ncut'][k]]
        handed += new.tolist()
        assert np.array_equal(w['store_pi'][new], p['selected_pi'][:took]) and np.all(w['vstat'][k, -kc:][p['nc0']:w['ncut'][k]] == 1)
        # rows past the slab's fill are as they were
        assert np.array_equal(w['slab_pi'][k, st1[F['slab_n'], k]:], s['slab_pi'][k, st1[F['slab_n'], k]:])
        assert np.array_equal(w['slab_pi'][k, :st0[F['slab_n'], k]], s['slab_pi'][k, :st0[F['slab_n'], k]])
    assert handed == list(range(count0, count0 + len(handed))) and len(handed) == min(w['attempts'], w['store_room'])
    assert w['store_count'][0] == count0 + w['attempts']
    rest = np.setdiff1d(np.arange(cap), handed)
    assert np.array_equal(w['store_pi'][rest], s['store_pi'][rest]) and np.array_equal(w['store_pi0'][rest], s['store_pi0'][rest])
    assert w['counters'][0] == s['counters'][0] and w['counters'][3] == s['counters'][3]


def test_cases_cover_every_path():
    """Computed from the restatement alone: what the GPU test compares the kernels on.  A generator change that loses a
    path fails here."""
    total = collections.Counter()
    by_case = {}
    for name in ref.CASES:
        s, w = ref.case(name)
        p = collections.Counter({k: v for k, v in w['paths'].items() if v > 0})
        p['B_%d' % s['B']] += 1
        by_case[name] = p
        total.update(p)
    need = ['B_1', 'B_2', 'B_3', 'B_5', 'B_70', 'gather', 'gather_scattered', 'gather_largest_last',
            'status_0', 'status_1', 'status_2', 'status_3', 'mip_feasible', 'stalled_on_entry', 'rounds_at_max', 'rounds_one_below_max',
            'obj_at_bound', 'obj_ulp_below_bound', 'was_inactive', 'was_active', 'change_ulp_below_tol', 'change_at_tol', 'change_ulp_above_tol',
            'zero_over_zero', 'x_over_zero', 'objective_inf', 'stalls_now', 'ncut_0', 'ncut_1', 'ncut_63', 'ncut_64', 'ncut_5',
            'list_full_kc64', 'list_full_kc5', 'remove_none', 'remove_all', 'remove_first_only', 'remove_last_only', 'remove_lane_63',
            'remove_alternating', 'dual_negative_zero', 'dual_subnormal_kept', 'dual_nan_kept', 'tableau_after_removal', 'tableau_without_dump',
            # generate
            'inactive', 'not_square', 'cut_rows', 'no_cut_rows', 'n_odd', 'n_even', 'n_plus_ms_odd', 'n_plus_ms_even',
            'fold_le_64', 'fold_gt_64', 'fold_1024', 'slab_room', 'slab_exact_fit', 'slab_overflow_by_1', 'slab_already_full',
            'pool_with_holes', 'pool_empty', 'pool_of_2040', 'empty_support_row', 'support_above_limit', 'rejected_parallel',
            'rejected_large_coefficient', 'terminator_0', 'terminator_1', 'terminator_2', 'terminator_3',
            'selects_all', 'selects_first_only', 'selects_last_only', 'selects_some', 'list_room', 'list_room_0', 'list_room_short_1',
            'list_room_exact', 'store_room', 'store_room_0', 'store_room_short_1', 'store_room_exact', 'resolve_set_on_entry']
    need += ['fold_rows_%d' % r for r in (1, 2, 63, 64, 65, 128, 129, 572)]
    assert [k for k in need if total[k] <= 0] == []
    # ... and every name the restatement counts is one this list knows (a new path gets a case and a line here)
    loose = ('ncut_', 'fold_rows_', 'list_room_short_', 'store_room_short_', 'slab_overflow_by_', 'remove_mixed')
    assert [k for k in total if k not in need and not k.startswith(loose)] == []
    # the named cases hold what their names say
    c = by_case
    assert c['begin-gather-largest-last']['gather_largest_last'] and c['begin-gather-largest-last']['gather_scattered']
    assert c['begin-B1-kc64-round0-dump1-gather0-off30']['remove_lane_63'] and c['begin-B1-kc64-round0-dump1-gather0-off30']['remove_last_only']
    assert c['begin-B1-kc64-round0-dump1-gather0-off14']['remove_all'] and c['begin-B1-kc64-round0-dump1-gather0-off14']['ncut_64']
    for rows in (1, 2, 63, 64, 65, 128, 129):
        assert c['generate-fold-%d-rows' % rows]['fold_rows_%d' % rows], rows
    assert c['generate-fold-1024x512-above-64KiB']['fold_1024'] and c['generate-fold-1024x512-above-64KiB']['cut_rows']
    assert c['generate-slab-exact']['slab_exact_fit'] == 2 and c['generate-slab-over1']['slab_overflow_by_1'] == 2 and c['generate-slab-full']['slab_already_full'] == 2
    assert c['generate-k3-holes']['pool_with_holes'] == 2 and c['generate-k3-holes']['rejected_parallel'] and c['generate-k3-holes']['empty_support_row']
    assert c['generate-k3-holes']['rejected_large_coefficient'] and c['generate-k3-maxnz1']['support_above_limit']
    assert all(c['generate-k3-terminators']['terminator_%d' % t] for t in range(4))
    assert c['generate-k3-kmax2040']['pool_of_2040'] and c['generate-k3-kmax2040']['slab_already_full']
    for B in (1, 3):
        assert c['generate-apply-list0-B%d' % B]['list_room_0'] == B and c['generate-apply-list1-B%d' % B]['list_room_short_1'] == B
        assert c['generate-apply-listexact-B%d' % B]['list_room_exact'] == B and c['generate-apply-store0-B%d' % B]['store_room_0']
        assert c['generate-apply-store1-B%d' % B]['store_room_short_1'] and c['generate-apply-storeexact-B%d' % B]['store_room_exact']
        assert c['generate-apply-both-B%d' % B]['list_room_short_2'] == B and any(k.startswith('store_room_short') for k in c['generate-apply-both-B%d' % B])
        assert c['generate-apply-select-first-B%d' % B]['selects_first_only'] == B and c['generate-apply-select-last-B%d' % B]['selects_last_only'] == B
        assert c['generate-apply-select-all-B%d' % B]['selects_all'] == B and c['generate-apply-resolve-in-B%d' % B]['resolve_set_on_entry'] == B
    for shape in ('65x33', '64x32', '64x33'):
        assert c['generate-sweep-%s-mixed' % shape]['inactive'] and c['generate-sweep-%s-mixed' % shape]['not_square']
        assert c['generate-sweep-%s-all' % shape]['list_room_0'] and c['generate-sweep-%s-all' % shape]['no_cut_rows']
    assert c['generate-sweep-65x33-all']['n_odd'] and c['generate-sweep-64x32-all']['n_plus_ms_even'] and c['generate-sweep-64x33-all']['n_plus_ms_odd']
    assert c['generate-sweep-64x33-all']['n_even']
    # the two tableaux of a real solve make cuts, and K3 takes some
    for name in ('generate-real-root', 'generate-real-resolved'):
        s, w = ref.case(name)
        assert w['k2_ncuts'][0] > 0 and w['k3_nadded'][0] > 0 and w['ncut'][0] > s['ncut'][0], name
    assert ref.case('generate-real-resolved')[0]['ncut'][0] == 3
