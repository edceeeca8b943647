"""The device finish on a caller's step (include/mipx_finish.h), the parts that need no GPU: the header against the
ctypes table and the exported symbols, the three records against the NumPy dtypes of the wrapper, and the restatement
the kernels are compared with (tests/support/finish_reference.py): hand-worked steps, its invariants on every case, and
that the cases reach every path the GPU test is there for."""
import collections
import os
import shutil
import subprocess

import numpy as np
import pytest

from simple_mip_solver_amd import _ffi
from tests.support import finish_reference as ref
from tests.support.abi_check import agrees, prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ['mipx_finish_step_batch', 'mipx_pc_apply_batch']
INF = float('inf')


def test_finish_header_and_signature_table_agree():
    protos = prototypes('mipx_finish.h')
    assert sorted(protos) == sorted(_ffi.FINISH_SYMBOLS) == sorted(NAMES)
    for name, (ret, params) in protos.items():
        restype, argtypes = _ffi._FINISH_SIGNATURES[name]
        assert agrees(ret, restype), name
        assert len(params) == len(argtypes), name
        for k, (decl, ctype) in enumerate(zip(params, argtypes)):
            assert agrees(decl, ctype), f'{name} parameter {k} is `{decl}`, the table says {ctype}'


def test_new_symbols_overlap_no_existing_list():
    old = set()
    for attr in dir(_ffi):
        if attr.endswith('SYMBOLS') and attr != 'FINISH_SYMBOLS':
            old |= set(getattr(_ffi, attr))
    assert old and not set(_ffi.FINISH_SYMBOLS) & old


def test_mipx_h_includes_the_header_and_keeps_its_version():
    text = open(os.path.join(ROOT, 'include', 'mipx.h')).read()
    assert '#include "mipx_finish.h"' in text
    assert _ffi.lib().mipx_abi_version() == 1
    # the header says what it is
    assert 'TEST SCAFFOLDING' in open(os.path.join(ROOT, 'include', 'mipx_finish.h')).read()


def test_library_exports_the_entries():
    L = _ffi.lib()
    for name in _ffi.FINISH_SYMBOLS:
        assert hasattr(L, name), name
        assert getattr(L, name).restype is _ffi._FINISH_SIGNATURES[name][0]


def test_c_entries_refuse_null_arguments():
    L = _ffi.lib()
    assert L.mipx_finish_step_batch(None, 5, 3, 1, 0, 0, 0, 16, *([None] * 7), 4, *([None] * 14)) == -1   # MIPX_EINVAL
    assert L.mipx_pc_apply_batch(None, 5, 0, *([None] * 7)) == -1


def test_no_product_code_calls_the_scaffolding():
    pkg = os.path.join(ROOT, 'simple_mip_solver_amd')
    for base, _, files in os.walk(pkg):
        for f in files:
            if f.endswith('.py') and f != '_ffi.py':
                text = open(os.path.join(base, f)).read()
                assert 'finish_step_batch' not in text and 'pc_apply_batch' not in text, f


def test_the_finish_kernels_are_launched_from_one_place():
    csrc = os.path.join(ROOT, 'simple_mip_solver_amd', 'csrc')
    hits = [(f, line.strip()) for f in sorted(os.listdir(csrc)) if f.endswith(('.h', '.hip'))
            for line in open(os.path.join(csrc, f)) if 'hipLaunchKernelGGL' in line and 'finish_' in line]
    assert {f for f, _ in hits} == {'tree_engine.hip.h'}
    assert sum('finish_write<' in line for _, line in hits) == 3      # (the dispatch on n, in enqueue_finish)
    assert sum('finish_scan' in line for _, line in hits) == 1


def test_records_match_the_dtypes(tmp_path):
    cxx = os.environ.get('CXX') or shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.fail('no host C++ compiler (c++, g++ or clang++) to build the layout check with')
    order = {'OpenEntry': ('key', 'bval', 'slot', 'depth', 'bidx_dir', 'anchor'),
             'PcSample': ('var_dir', 'status', 'obj', 'bound', 'vc'),
             'FinishSummary': ('host_path', 'n_open', 'n_dead', 'n_samples', 'unbounded', 'incumbent_pos', 'n_deferred', 'pad0',
                               'evaluated', 'dives', 'pivots', 'closed_min', 'primal', 'primal_before', 'pad')}
    dtypes = {'OpenEntry': _ffi.OPEN_ENTRY_DTYPE, 'PcSample': _ffi.PC_SAMPLE_DTYPE, 'FinishSummary': _ffi.FINISH_SUMMARY_DTYPE}
    args = []
    for name, dt in dtypes.items():
        assert dt.names == order[name]
        args += [name, str(dt.itemsize)] + [str(dt.fields[f][1]) for f in dt.names]
    assert set(ref.SUMMARY_FIELDS) == set(order['FinishSummary']) - {'pad0', 'pad'}
    exe = str(tmp_path / 'finish_layout_check')
    subprocess.run([cxx, '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror', '-I', os.path.join(ROOT, 'simple_mip_solver_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'support', 'finish_layout_check.cpp'), '-o', exe], check=True)
    run = subprocess.run([exe] + args, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert ' 0 failed' in run.stdout and 'finish_layout: 29 checks' in run.stdout, run.stdout
    # ... and it does fail on a dtype that is off
    bad = subprocess.run([exe] + args[:3] + ['4'] + args[4:], capture_output=True, text=True)
    assert bad.returncode == 1 and 'bval' in bad.stderr


# ---- hand-worked steps -------------------------------------------------------------------------------------------
def tiny(B, dive, rule, primal, chains, par=None):
    """A step of n = 2, m = 1 from per-chain lists of levels.  A level is a dict of the fields that differ from an optimal,
    fractional node without a candidate (status 0, mipf 0, nprobe 0, bidx -1, dvar -1).  The batch sits in the pool rows
    0..B-1 with l = (0, 0), u = (9, 9); chain k's budget is the rows B + per k .. B + per k + per - 1; npiv of a position is
    the position + 1."""
    L, per = dive + 1, 2 * (1 + dive)
    rows = B + per * B + 1
    s = dict(n=2, m=1, B=B, dive=dive, rule=rule, ask_count=0, ask_cap=16, primal=primal)
    ints = dict(status=0, bidx=-1, mipf=0, nprobe=0, dvar=-1, ddir=0)
    for key, fill in ints.items():
        s[key] = np.full((L, B), fill, np.int32)
    s['status'][1:] = -1
    s['npiv'] = (np.arange(L * B, dtype=np.int32) + 1).reshape(L, B)
    for key in ('obj', 'bval', 'dval'):
        s[key] = np.zeros((L, B))
    for k, levels in enumerate(chains):
        for p, fields in enumerate(levels):
            s['status'][p, k] = 0
            for key, v in fields.items():
                s[key][p, k] = v
    s['vout'] = (np.arange(L * B * 3) % 100).astype(np.int8).reshape(L * B, 3)
    s['slot'] = np.arange(B, dtype=np.int32)
    s['budget'] = (B + np.arange(B * per, dtype=np.int32)).reshape(B, per)
    par = par or [(-1, 0, 0.0, 0.0)] * B          # (b_idx, b_dir, dual_bound, b_val) of the batch's nodes
    s['par_i'] = np.array([[q[0] for q in par], [q[1] for q in par], [10 * (k + 1) for k in range(B)], [k + 100 for k in range(B)]], np.int32)
    s['par_d'] = np.array([[q[2] for q in par], [q[3] for q in par]], np.float64)
    s['pool_l'] = np.full((rows, 2), ref.SENTINEL_BOUND); s['pool_u'] = np.full((rows, 2), ref.SENTINEL_BOUND)
    s['pool_v'] = np.full((rows, 3), ref.SENTINEL_BASIS, np.int8)
    s['pool_l'][:B], s['pool_u'][:B], s['pool_v'][:B] = 0.0, 9.0, 1
    s['cost_l'], s['cost_r'] = np.array([1.0, 0.0]), np.array([0.0, 4.0])
    s['has'], s['times'], s['own'] = np.array([1, 1], np.uint8), np.array([1, 0, 0, 3], np.int32), np.zeros(8)
    return s


def records(a):
    return [tuple(r) for r in a.tolist()]


def tie_step(primal):
    return tiny(3, 1, 0, primal, [
        [dict(obj=5.0, dvar=0, ddir=0, dval=1.5), dict(obj=7.0, mipf=1)],     # dives left, ends in an integral node of 7
        [dict(obj=7.0, mipf=1)],                                               # an integral node of 7 again
        [dict(obj=6.0, bidx=1, bval=0.25)]])                                   # branches without a dive


def test_hand_worked_tie_keeps_the_first_leaf():
    w = ref.finish_step(tie_step(INF))
    assert w['summary'] == dict(host_path=0, n_open=3, n_dead=9, n_samples=0, unbounded=0, incumbent_pos=3, n_deferred=0,
                                evaluated=4, dives=1, pivots=1 + 4 + 2 + 3, closed_min=7.0, primal=7.0, primal_before=INF)
    assert records(w['open']) == [(5.0, 1.5, 4, 11, 1, 100), (6.0, 0.25, 11, 31, 2, 102), (6.0, 0.25, 12, 31, 3, 102)]
    assert w['dead'].tolist() == [3, 5, 6, 7, 8, 9, 10, 13, 14]
    # the child records: the parent's bounds with the one bound of the branch, the basis the parent's LP ended with
    assert w['pool_l'][4].tolist() == [2.0, 0.0] and w['pool_u'][4].tolist() == [9.0, 9.0] and w['pool_v'][4].tolist() == [0, 1, 2]
    assert w['pool_l'][11].tolist() == [0.0, 0.0] and w['pool_u'][11].tolist() == [9.0, 0.0]
    assert w['pool_l'][12].tolist() == [0.0, 1.0] and w['pool_u'][12].tolist() == [9.0, 9.0] and w['pool_v'][12].tolist() == [6, 7, 8]
    untouched = [r for r in range(16) if r not in (0, 1, 2, 4, 11, 12)]
    assert np.all(w['pool_l'][untouched] == ref.SENTINEL_BOUND) and np.all(w['pool_v'][untouched] == ref.SENTINEL_BASIS)
    assert w['paths']['leaf_tie'] == 1 and w['paths']['leaf_tie_other_range'] == 1     # (B <= 1024: a range is one chain)


def test_hand_worked_leaf_at_the_incumbent_is_no_improvement():
    w = ref.finish_step(tie_step(7.0))
    assert w['summary'] == dict(host_path=0, n_open=3, n_dead=9, n_samples=0, unbounded=0, incumbent_pos=-1, n_deferred=0,
                                evaluated=4, dives=1, pivots=10, closed_min=7.0, primal=7.0, primal_before=7.0)
    assert w['dead'].tolist() == [3, 5, 6, 7, 8, 9, 10, 13, 14] and w['primal'] == 7.0
    assert w['paths']['leaf_equal_incumbent'] == 2 and w['paths']['no_improvement'] == 1


def mixed_step():
    return tiny(4, 1, 1, 10.0, [
        [dict(obj=3.0, mipf=1)],                                                      # the incumbent: 3
        [dict(obj=2.0, dvar=1, ddir=1, dval=0.5), dict(obj=4.0, bidx=0, bval=0.5)],   # below it, its dive child is not
        [dict(obj=1.0, dvar=0, ddir=1, dval=0.5, bidx=0, bval=2.75)],                 # a dive child that was not solved
        [dict(obj=0.5, nprobe=2, bidx=1, bval=0.5)]],                                 # filed probe requests: the host's
        par=[(0, 0, 2.0, 1.5), (-1, 0, 0.0, 0.0), (1, 1, 1.5, 0.25), (0, 1, 0.0, 0.5)])


def test_hand_worked_prune_dropped_child_and_deferred_chain():
    w = ref.finish_step(mixed_step())
    assert w['summary'] == dict(host_path=0, n_open=3, n_dead=13, n_samples=3, unbounded=0, incumbent_pos=0, n_deferred=1,
                                evaluated=4, dives=1, pivots=1 + 2 + 6 + 3, closed_min=3.0, primal=3.0, primal_before=10.0)
    assert records(w['open']) == [(2.0, 0.5, 8, 21, 2, 101), (1.0, 2.75, 12, 31, 0, 102), (1.0, 2.75, 13, 31, 1, 102)]
    assert w['dead'].tolist() == [4, 5, 6, 7, 9, 10, 11, 14, 15, 16, 17, 18, 19]
    assert w['pool_u'][8].tolist() == [9.0, 0.0] and w['pool_u'][12].tolist() == [2.0, 9.0] and w['pool_l'][13].tolist() == [3.0, 0.0]
    # the samples: the branch that made chain 0's node; chain 1's dive child; the branch that made chain 2's node, whose
    # value lies below its parent's bound
    assert records(w['samples']) == [(0, 0, 3.0, 2.0, 0.5), (3, 0, 4.0, 2.0, 0.5), (3, 0, 1.0, 1.5, 0.75)]
    assert w['sample_keys'].tolist() == [0, 3, 3]
    # column 0 left: (1 * 1 + (3 - 2) / 0.5) / 2;  column 1 right: (4 * 3 + 2 / 0.5) / 4 = 4, then (4 * 4 + 0) / 5
    assert w['cost_l'].tolist() == [1.5, 0.0] and w['cost_r'].tolist() == [0.0, 3.2]
    assert w['times'].tolist() == [2, 0, 0, 5] and w['has'].tolist() == [1, 1]
    assert w['own'].tolist() == [2.0, 0.0, 0.0, 4.0, 1.0, 0.0, 0.0, 2.0]
    p = w['paths']
    assert p['pruned_mid_chain_by_earlier_chain'] == 1 and p['dive_dropped_unsolved'] == 1 and p['deferred_beside_finished'] == 1
    assert p['sample_negative_change'] == 1


def test_hand_worked_ask_cap_leaves_the_step_to_the_host():
    s = mixed_step()
    s['ask_count'] = 17
    w = ref.finish_step(s)
    assert w['summary'] == dict(host_path=1) and w['primal'] == 10.0
    assert len(w['open']) == len(w['dead']) == len(w['samples']) == 0
    for k in ('pool_l', 'pool_u', 'pool_v', 'cost_l', 'cost_r', 'has', 'times', 'own'):
        assert np.array_equal(w[k], s[k]), k
    s['ask_count'] = 16      # (as many as the list holds: not the host's)
    assert ref.finish_step(s)['summary']['host_path'] == 0


def test_hand_worked_recurrence_of_three_samples():
    samples = np.array([(5, 0, 5.0, 3.0, 0.5),      # (2 * 1 + 2 / 0.5) / 2 = 3
                        (5, 2, 9.0, 1.0, 0.5),      # counts without a cost: the mean stays, times 3
                        (5, 3, 1.0, 2.0, 0.25)],    # below the bound: (3 * 3 + 0) / 4
                       _ffi.PC_SAMPLE_DTYPE)
    cl, cr, has, times, own = ref.apply_samples(samples, np.zeros(3), np.array([0.0, 0.0, 2.0]), np.zeros(3, np.uint8),
                                                np.array([0, 0, 0, 0, 0, 1], np.int32), np.zeros(12))
    assert cr.tolist() == [0.0, 0.0, 2.25] and cl.tolist() == [0.0] * 3
    assert times.tolist() == [0, 0, 0, 0, 0, 4] and has.tolist() == [0, 0, 1]
    assert own.tolist() == [0.0] * 5 + [4.0 + 3.0 + 0.0] + [0.0] * 5 + [3.0]


# ---- the restatement on every case -------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(ref.CASES))
def test_invariants_of_the_restatement(name):
    s, w = ref.case(name)
    B, dive = s['B'], s['dive']
    per, sm = 2 * (1 + dive), w['summary']
    if sm['host_path']:
        assert sm == dict(host_path=1) and s['ask_count'] > s['ask_cap']
        return
    assert sm['n_open'] + sm['n_dead'] == per * B and sm['n_open'] == len(w['open']) and sm['n_dead'] == len(w['dead'])
    assert sorted(w['open']['slot'].tolist() + w['dead'].tolist()) == sorted(s['budget'].ravel().tolist())
    assert sm['evaluated'] - sm['dives'] == B - sm['n_deferred'] and 0 <= sm['dives'] <= dive * B
    assert sm['primal'] == min([s['primal']] + w['leaves']) == w['primal'] and sm['primal_before'] == s['primal']
    assert (sm['incumbent_pos'] >= 0) == (sm['primal'] < sm['primal_before'])
    if sm['incumbent_pos'] >= 0:
        pos = divmod(sm['incumbent_pos'], B)
        assert s['obj'][pos] == sm['primal'] and s['mipf'][pos] and s['status'][pos] in (0, 2)
    assert sm['n_deferred'] == int(np.sum(s['nprobe'][0] > 0))
    assert sm['n_samples'] == len(w['samples']) == len(w['sample_keys']) and (s['rule'] == 1 or sm['n_samples'] == 0)
    # rows nobody was given hold the sentinels, the batch's own rows are as they were
    given = np.zeros(len(s['pool_l']), bool)
    given[w['open']['slot']] = True
    assert np.all(w['pool_l'][~given] == s['pool_l'][~given]) and np.all(w['pool_v'][~given] == s['pool_v'][~given])
    spare = np.setdiff1d(np.arange(len(given)), np.concatenate([s['slot'], s['budget'].ravel()]))
    assert len(spare) and np.all(w['pool_u'][spare] == ref.SENTINEL_BOUND)
    # a child differs from its parent chain's node in the bounds of the columns branched on, and only there
    if sm['n_open']:
        assert np.all(w['pool_l'][given] != ref.SENTINEL_BOUND) and np.all(w['pool_v'][given] != ref.SENTINEL_BASIS)
        assert np.all(w['open']['depth'] >= 1)
    if s['rule'] == 1:
        assert int(w['times'].sum() - s['times'].sum()) == sm['n_samples']
        assert w['own'][2 * s['n']:].sum() - s['own'][2 * s['n']:].sum() == sm['n_samples']


def test_cases_cover_every_path():
    """Computed from the restatement alone: what the GPU test compares the kernels on.  A generator change that loses a
    path fails here."""
    total = collections.Counter()
    by_case = {}
    for name in ref.CASES:
        s, w = ref.case(name)
        p = collections.Counter(w['paths'])
        B, n, nv = s['B'], s['n'], s['n'] + s['m']
        p['C_%d' % -(-B // 1024)] += 1
        p['NE_%d' % (1 if n <= 256 else 2 if n <= 512 else 4)] += 1
        if len(w['open']):
            p['vout_words' if nv % 4 == 0 else 'vout_bytes'] += 1
        if B % 1024 and -(-B // 1024) > 1 and 1023 * -(-B // 1024) >= B:
            p['last_thread_owns_no_chain'] += 1
        if s['rule'] == 1 and not w['summary']['host_path']:
            p['samples_%d' % w['summary']['n_samples']] += 1
            per_entry = collections.Counter(w['sample_keys'].tolist())
            if len(per_entry) == 1 and w['summary']['n_samples'] > 1024:
                p['one_entry_owns_every_sample'] += 1
        by_case[name] = p
        total.update(p)
    need = ['leaf_tie_same_range', 'leaf_tie_other_range', 'leaf_equal_incumbent', 'no_improvement', 'improvement',
            'pruned_mid_chain_by_earlier_chain', 'dive_dropped_unsolved', 'dive_dropped_probes', 'status_unbounded',
            'nothing_open', 'primal_inf', 'primal_finite', 'deferred_beside_finished', 'ask_cap', 'dive_left', 'dive_right',
            'C_1', 'C_2', 'C_3', 'C_5', 'NE_1', 'NE_2', 'NE_4', 'vout_words', 'vout_bytes', 'last_thread_owns_no_chain',
            'sample_costed', 'sample_count_only', 'sample_negative_change', 'one_entry_owns_every_sample']
    need += ['samples_%d' % c for c in ref.SAMPLE_COUNTS]
    need += ['branch_column_%d' % c for c in (0, 255, 256, 511, 512, 1023)]
    assert [k for k in need if total[k] <= 0] == []
    # the named cases hold what their names say
    c = by_case
    assert c['outcome-tie-same-range']['leaf_tie_same_range'] and ref.case('outcome-tie-same-range')[1]['summary']['incumbent_pos'] == 2049 + 300
    assert c['outcome-tie-across-ranges']['leaf_tie_other_range'] and ref.case('outcome-tie-across-ranges')[1]['summary']['incumbent_pos'] == 3 * 2049 + 4
    assert c['outcome-tie-small']['leaf_tie'] and ref.case('outcome-tie-small')[1]['summary']['incumbent_pos'] == 7 + 2
    assert c['outcome-leaf-equals-incumbent']['leaf_equal_incumbent'] >= 3 and c['outcome-leaf-equals-incumbent']['no_improvement']
    assert c['outcome-prune-mid-plunge']['pruned_mid_chain_by_earlier_chain'] >= 2
    for name in ('outcome-all-closed', 'outcome-all-infeasible'):
        assert c[name]['nothing_open'] and ref.case(name)[1]['summary']['n_open'] == 0
    assert c['outcome-all-closed']['C_2'] and c['outcome-unbounded']['status_unbounded'] and c['outcome-deferred']['deferred_beside_finished']
    assert c['outcome-dropped-dive-children']['dive_dropped_unsolved'] and c['outcome-dropped-dive-children']['dive_dropped_probes']
    assert c['outcome-ask-cap']['ask_cap'] and not c['outcome-ask-at-cap']['ask_cap']
    assert c['samples-1025-one-owner']['one_entry_owns_every_sample']
    # every column case plunges both ways through every register edge it has, in one chain
    for n in (256, 257, 512, 513, 1024):
        p = c['columns-n%d' % n]
        assert p['dive_left'] >= 8 and p['dive_right'] >= 8
        assert all(p['branch_column_%d' % e] for e in (0, 255, 256, 511, 512, n - 1) if e < n), n
    # the widths: every B at both shapes, every depth, both rules, and chains that dive where there are levels
    for B in ref.WIDTHS:
        for name, p in c.items():
            if name.startswith('width-B%d-' % B) and '-dive0' not in name and B >= 2:
                assert p['dive_left'] + p['dive_right'] > 0, name
    assert sum(name.startswith('width-') for name in c) == len(ref.WIDTHS) * 2 * 3 * 2
