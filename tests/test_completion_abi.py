"""The completion over the continuous columns (include/mipx_complete.h), the parts that need no GPU: the header against
the ctypes table and the exported symbols, what BranchAndBound refuses at construction, the layout of the option's step
buffer, and the NumPy restatement of the algorithm (tests/support/completion_reference.py) around the oracle's node LP:
its points certified, its objectives against scipy's linprog on the same fixed integers, its verdicts against HiGHS."""
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from scipy.optimize import linprog

from simple_mip_solver_amd import BranchAndBound, PseudoCostBranchNode, _ffi
from tests.support import completion_reference as ref
from tests.support import heuristic_reference as heur
from tests.support.abi_check import agrees, prototypes
from tests.support.example_models import model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ['mipx_complete_batch', 'mipx_tree_set_completion', 'mipx_tree_completion_stats']


def test_completion_header_and_signature_table_agree():
    protos = prototypes('mipx_complete.h')
    assert sorted(protos) == sorted(_ffi.COMPLETE_SYMBOLS) == sorted(NAMES)
    for name, (ret, params) in protos.items():
        restype, argtypes = _ffi._COMPLETE_SIGNATURES[name]
        assert agrees(ret, restype), name
        assert len(params) == len(argtypes), name
        for k, (decl, ctype) in enumerate(zip(params, argtypes)):
            assert agrees(decl, ctype), f'{name} parameter {k} is `{decl}`, the table says {ctype}'


def test_new_symbols_overlap_no_existing_list():
    old = set(_ffi.SYMBOLS) | set(_ffi.SPILL_SYMBOLS) | set(_ffi.CUTMIG_SYMBOLS) | set(_ffi.DUALFN_SYMBOLS) | \
        set(_ffi.TREEREC_SYMBOLS) | set(_ffi.CGLP_SYMBOLS) | set(_ffi.RESTART_SYMBOLS) | set(_ffi.HEUR_SYMBOLS) | \
        set(_ffi.PROP_SYMBOLS) | set(_ffi.RCFIX_SYMBOLS) | set(_ffi.OBJSTEP_SYMBOLS) | set(_ffi.LSEARCH_SYMBOLS) | \
        set(_ffi.FIXPROP_SYMBOLS) | set(_ffi.WREPAIR_SYMBOLS) | set(_ffi.CUBE_SYMBOLS)
    assert not set(_ffi.COMPLETE_SYMBOLS) & old
    assert len(_ffi._SIGNATURES) == 70   # (the new entries have a table of their own)


def test_mipx_h_includes_the_header_and_declares_nothing_new_itself():
    text = open(os.path.join(ROOT, 'include', 'mipx.h')).read()
    assert '#include "mipx_complete.h"' in text
    assert not re.search(r'mipx_(tree_)?(set_)?complet', re.sub(r'#include "mipx_complete.h".*', '', text))
    assert _ffi.lib().mipx_abi_version() == 1


def test_library_exports_the_entries():
    L = _ffi.lib()
    for name in _ffi.COMPLETE_SYMBOLS:
        assert hasattr(L, name), name
        assert getattr(L, name).restype is _ffi._COMPLETE_SIGNATURES[name][0]


def test_stats_keys_and_status_codes_cover_the_header():
    text = open(os.path.join(ROOT, 'include', 'mipx_complete.h')).read()
    assert [int(k) for k in re.findall(r'\[(\d)\] ', text)] == list(range(8))
    assert _ffi.COMPLETE_STATS_KEYS == ('points', 'completed', 'infeasible', 'failed', 'rescued', 'incumbents', 'pivots', 'kernel_us')
    codes = {name.lower(): int(v) for name, v in
             re.findall(r'#define MIPX_COMPLETE_(COMPLETED|INFEASIBLE|LIMIT|SKIPPED|REJECTED) (\d)', text)}
    assert codes == {v: k for k, v in _ffi.COMPLETE_STATUS.items()} and len(codes) == 5
    assert (ref.COMPLETED, ref.INFEASIBLE, ref.LIMIT, ref.SKIPPED, ref.REJECTED) == \
        tuple(codes[k] for k in ('completed', 'infeasible', 'limit', 'skipped', 'rejected'))
    # COMPLETED and SKIPPED are the heuristic's feasible and skipped, as the cube's FOUND and SKIPPED are
    assert _ffi.HEUR_STATUS[codes['completed']] == 'feasible' and _ffi.HEUR_STATUS[codes['skipped']] == 'skipped'
    assert _ffi.CUBE_STATUS[codes['completed']] == 'found' and _ffi.CUBE_STATUS[codes['skipped']] == 'skipped'
    assert _ffi.DEFAULT_COMPLETION_TOL == ref.CTOL == 1e-6


def test_c_entries_refuse_null_arguments():
    L = _ffi.lib()
    assert L.mipx_complete_batch(None, 0, *([None] * 4), 0, None, 1e-6, None, *([None] * 4)) == -1   # MIPX_EINVAL
    assert L.mipx_tree_set_completion(None, 1) == -1
    assert L.mipx_tree_completion_stats(None, None) == -1


def test_step_buffer_layout_matches_the_engine(tmp_path):
    cxx = os.environ.get('CXX') or shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.fail('no host C++ compiler (c++, g++ or clang++) to build the layout check with')
    exe = str(tmp_path / 'completion_layout_check')
    subprocess.run([cxx, '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror', '-I', os.path.join(ROOT, 'simple_mip_solver_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'support', 'completion_layout_check.cpp'), '-o', exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert ' 0 failed' in run.stdout, run.stdout


# ---- what the constructor refuses ------------------------------------------------------------------------------
def build(**extra):
    kw = dict(pseudo_costs={}, frontier_batch=4, gomory_cuts=False, primal_heuristic=True, complete_continuous=True)
    kw.update(extra)
    return BranchAndBound(model('small_branch'), PseudoCostBranchNode, **kw)


@pytest.mark.parametrize('value', [False, 0, 1, 2.5, 'on'])
def test_complete_continuous_value(value):
    with pytest.raises(ValueError, match='complete_continuous is None or True'):
        build(complete_continuous=value)


def test_completion_needs_the_heuristic():
    with pytest.raises(ValueError, match='complete_continuous needs primal_heuristic'):
        build(primal_heuristic=None)
    with pytest.raises(AssertionError, match='primal_heuristic needs frontier_batch'):
        build(frontier_batch=None)
    with pytest.raises(AssertionError, match='primal_heuristic needs gomory_cuts=False'):
        build(gomory_cuts=True)
    with pytest.raises(AssertionError, match='primal_heuristic cannot be combined with comm'):
        build(comm=object())


def test_option_is_off_by_default_and_works_beside_the_others():
    on = build()
    assert on._complete_continuous is True and on.completion_stats is None and on._given['complete_continuous'] is True
    plain = build(complete_continuous=None)
    assert plain._complete_continuous is None and plain._given['complete_continuous'] is None and plain.completion_stats is None
    assert BranchAndBound(model('small_branch'), PseudoCostBranchNode, pseudo_costs={})._complete_continuous is None
    assert 'complete_continuous' in BranchAndBound._restart_overrides and 'primal_heuristic' in BranchAndBound._restart_overrides
    assert build(propagate=True, reduced_cost=True, objective_step=True, local_search=True, host_spill=1 << 24, dive=8,
                 anchor=False)._complete_continuous is True
    assert build(tree_record=True)._complete_continuous is True and build(dual_function=True)._complete_continuous is True
    assert build(fix_propagate=True, cube_search=True)._complete_continuous is True
    assert build(weighted_repair=True, cube_search=7, local_search=True)._complete_continuous is True


def test_restart_inherits_the_option_and_drops_it_with_the_heuristic(monkeypatch):
    from simple_mip_solver_amd.lp import CyLPArray
    src = build(tree_record=True, cube_search=True)
    src.status = 'optimal'
    seeded = []
    monkeypatch.setattr(BranchAndBound, '_seed_native', lambda self, source: seeded.append(self))
    b = CyLPArray(np.asarray(src.root_node.lp.constraints[0].lower, dtype=np.float64).copy())
    kept = src.restart(b)
    assert kept._complete_continuous is True and kept._primal_heuristic is True and kept._cube_search is True
    new = src.restart(b, primal_heuristic=None)
    assert new._primal_heuristic is None and new._complete_continuous is None and new._cube_search is None and seeded == [kept, new]
    off = src.restart(b, complete_continuous=None)
    assert off._complete_continuous is None and off._cube_search is True
    with pytest.raises(ValueError, match='complete_continuous needs primal_heuristic'):
        src.restart(b, primal_heuristic=None, complete_continuous=True)


# ---- the restatement around the oracle's node LP ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def run(family, n, m, seed):
    """(instance, LP points, their rounded points and the frozen rounding's statuses and objectives, the restatement's
    batch cold and warm) of one instance, made once."""
    inst = getattr(ref, family)(n, m, seed)
    A, b, c, l, u, ints = inst
    X, V, _, _ = ref.lp_points(inst, seed, 32, 4 if n >= 16 else 2)
    Xt, fobj, fstatus, _ = heur.round_repair_lift(A, b, c, l, u, ints, X)
    cold = ref.complete(A, b, c, l, u, ints, Xt, ref.oracle_lp(A, b, c))
    warm = ref.complete(A, b, c, l, u, ints, Xt, ref.oracle_lp(A, b, c), vstat=V)
    return inst, X, Xt, fstatus, fobj, cold, warm


def fixed_lp(inst, xt):
    """scipy's linprog on the LP with the integer columns fixed at xt's: an LP solver of its own."""
    A, b, c, l, u, ints = inst
    lo, hi = l.copy(), u.copy()
    lo[ints] = xt[ints]
    hi[ints] = xt[ints]
    return linprog(c, A_ub=-A, b_ub=-b, bounds=list(zip(lo, hi)), method='highs')


CASES = [(f, n, m, s) for f in ('mixed', 'packing') for n, m in ((8, 4), (40, 20)) for s in (0, 1, 2)]


@pytest.mark.parametrize('family,n,m,seed', CASES)
def test_completed_points_are_certified_and_optimal_for_their_integers(family, n, m, seed):
    inst, X, Xt, fstatus, fobj, cold, warm = run(family, n, m, seed)
    A, b, c, l, u, ints = inst
    rest = np.setdiff1d(np.arange(n), ints)
    print(family, n, m, seed, 'frozen feasible', int((fstatus == 0).sum()), 'completed', int((cold['status'] == 0).sum()),
          'status', np.bincount(cold['status'], minlength=5), 'pivots cold', cold['pivots'].mean(), 'warm', warm['pivots'].mean())
    assert np.array_equal(cold['status'], warm['status'])   # (correctness does not depend on the start)
    assert set(cold['status']) <= {ref.COMPLETED, ref.INFEASIBLE}   # (a rounded point is never skipped; no limit at these sizes)
    for o in (cold, warm):
        for p in range(len(Xt)):
            h = fixed_lp(inst, Xt[p])
            if o['status'][p] == ref.COMPLETED:
                heur.certify(A, b, c, l, u, ints, o['x'][p], o['obj'][p], tol=1e-6)
                assert np.array_equal(o['x'][p][ints], Xt[p][ints])   # (the integers are the heuristic's, to the bit)
                assert h.status == 0 and abs(o['obj'][p] - h.fun) <= 1e-9 * max(1.0, abs(h.fun)), (p, o['obj'][p], h.fun)
                if fstatus[p] == 0:   # (the frozen point is feasible for that LP: the optimum is no worse)
                    assert o['obj'][p] <= fobj[p] + 1e-9 * max(1.0, abs(fobj[p]))
            else:
                assert o['status'][p] == ref.INFEASIBLE and h.status == 2, (p, h.status)   # (INFEASIBLE agrees with HiGHS)
                assert np.array_equal(o['x'][p].view(np.int64), Xt[p].view(np.int64)) and o['obj'][p] == 0.0 and fstatus[p] != 0
        assert np.array_equal(o['x'][:, rest][o['status'] != 0].view(np.int64), Xt[:, rest][o['status'] != 0].view(np.int64))


def test_the_figures_of_the_issue_at_40_by_20():
    """The table the option was proposed with, at 40 x 20, with the points made as stated there (the root's LP point, then
    LPs with four random integer bounds moved to the floor or the ceil of the root value; 32 points per instance).
    What the procedure fixes is asserted as the table has it: the frozen rounding is feasible on 32 of 32 points of
    the packing family (seeds 1, 2) and on 0 of 32 of the mixed family (seeds 0, 1, 2); the completion ends feasible
    on 32 of 32 packing points, improving each by 4.0 to 7.4 on average, and on 32 of 32 mixed points at seed 0.  The
    table's 1 and 26 of 32 at mixed seeds 1 and 2 depend on which bounds were drawn, which it does not state: with
    numpy's default_rng(seed) drawing them this file gets 0 and 21 of 32, checked point by point against HiGHS
    above and here required to be what HiGHS gives on the same points: almost none at seed 1, most at seed 2."""
    for seed in (1, 2):
        inst, X, Xt, fstatus, fobj, cold, warm = run('packing', 40, 20, seed)
        done = cold['status'] == ref.COMPLETED
        gain = float(np.mean(fobj - cold['obj']))
        print('packing', seed, 'frozen', int((fstatus == 0).sum()), 'completed', int(done.sum()), 'mean gain', gain)
        assert int((fstatus == 0).sum()) == 32 and int(done.sum()) == 32
        assert 4.0 <= gain <= 7.4
    got = {}
    for seed in (0, 1, 2):
        inst, X, Xt, fstatus, fobj, cold, warm = run('mixed', 40, 20, seed)
        A, b, c, l, u, ints = inst
        highs = ref.complete(A, b, c, l, u, ints, Xt, ref.highs_lp(A, b, c))
        got[seed] = int((cold['status'] == ref.COMPLETED).sum())
        print('mixed', seed, 'frozen', int((fstatus == 0).sum()), 'completed', got[seed], 'with HiGHS', int((highs['status'] == 0).sum()))
        assert int((fstatus == 0).sum()) == 0
        assert np.array_equal(cold['status'], highs['status'])
    assert got[0] == 32 and got[1] <= 1 and 16 < got[2] < 32


def test_restatement_edges():
    A = np.array([[1.0, 1.0], [-1.0, -1.0]]); b = np.array([1.5, -3.0]); c = np.array([1.0, 2.0])
    l = np.zeros(2); u = np.array([5.0, np.inf])
    lp = ref.oracle_lp(A, b, c)
    # column 0 integer at 1: the LP puts column 1 at 0.5
    o = ref.complete(A, b, c, l, u, [0], [[1.0, 3.0]], lp)
    assert o['status'][0] == ref.COMPLETED and list(o['x'][0]) == [1.0, 0.5] and o['obj'][0] == 2.0
    # a fractional, an out-of-bounds and a masked point are skipped and come back as they are; 4 + x1 <= 3 is infeasible
    o = ref.complete(A, b, c, l, u, [0], [[1.5, 0.0], [6.0, 0.0], [1.0, 0.0], [4.0, 0.0]], lp, skip=[0, 0, 1, 0])
    assert list(o['status']) == [ref.SKIPPED, ref.SKIPPED, ref.SKIPPED, ref.INFEASIBLE]
    assert o['x'].tolist() == [[1.5, 0.0], [6.0, 0.0], [1.0, 0.0], [4.0, 0.0]] and not o['obj'].any() and not o['pivots'][:3].any()
    # every column integer: the LP only confirms or refutes the point
    o = ref.complete(A, b, c, l, [5.0, 5.0], [0, 1], [[1.0, 1.0], [0.0, 1.0]], lp)
    assert list(o['status']) == [ref.COMPLETED, ref.INFEASIBLE] and o['obj'][0] == 3.0
    # an LP function that calls a wrong point optimal is caught: REJECTED, the point unchanged
    liar = lambda L, U, V: dict(status=np.zeros(1, np.int32), x=np.array([[1.0, 0.0]]), npivots=np.ones(1, np.int32))
    o = ref.complete(A, b, c, l, u, [0], [[1.0, 3.0]], liar)
    assert o['status'][0] == ref.REJECTED and list(o['x'][0]) == [1.0, 3.0] and o['obj'][0] == 0.0 and o['pivots'][0] == 1
    # ... and within ctol it is not: row 0 short by 5e-7
    near = lambda L, U, V: dict(status=np.zeros(1, np.int32), x=np.array([[1.0, 0.4999995]]), npivots=np.ones(1, np.int32))
    assert ref.complete(A, b, c, l, u, [0], [[1.0, 3.0]], near)['status'][0] == ref.COMPLETED
    assert ref.complete(A, b, c, l, u, [0], [[1.0, 3.0]], near, ctol=0.0)['status'][0] == ref.REJECTED
    assert len(ref.complete(A, b, c, l, u, [0], np.zeros((0, 2)), lp)['status']) == 0
