"""The bound propagation (include/mipx_prop.h), the parts that need no GPU: the header against the ctypes table and
the exported symbols, what BranchAndBound refuses at construction, the NumPy restatement of the algorithm
(tests/support/propagation_reference.py) against brute force, and the input conditions of the GPU tests."""
import ctypes as C
import heapq
import itertools
import os
import re

import numpy as np
import pytest
from scipy.optimize import linprog

from simple_mip_solver_amd import BranchAndBound, PseudoCostBranchNode, _ffi
from simple_mip_solver_amd.generators import random_dense_milp_arrays
from tests.support import propagation_reference as ref
from tests.support.example_models import model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ['mipx_propagate_batch', 'mipx_tree_set_propagation', 'mipx_tree_propagation_stats']


def prop_prototypes():
    text = open(os.path.join(ROOT, 'include', 'mipx_prop.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    text = re.sub(r'^\s*#.*$', '', text, flags=re.M)
    found = re.findall(r'([\w ]+?[\s*]+)(mipx_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;', text)
    return {name: (ret.strip(), [p.strip() for p in args.split(',') if p.strip() not in ('', 'void')])
            for ret, name, args in found}


def test_propagation_header_and_signature_table_agree():
    scalars = {'int': C.c_int, 'int64_t': C.c_int64, 'size_t': C.c_size_t, 'double': C.c_double, 'void': None}

    def agrees(decl, ctype):
        if '*' in decl or '[' in decl:
            return ctype in (C.c_void_p, C.c_char_p) or (isinstance(ctype, type) and issubclass(ctype, C._Pointer))
        return ctype is scalars[decl.replace('const ', '').split()[0]]

    protos = prop_prototypes()
    assert sorted(protos) == sorted(_ffi.PROP_SYMBOLS) == sorted(NAMES)
    for name, (ret, params) in protos.items():
        restype, argtypes = _ffi._PROP_SIGNATURES[name]
        assert agrees(ret, restype), name
        assert len(params) == len(argtypes), name
        for k, (decl, ctype) in enumerate(zip(params, argtypes)):
            assert agrees(decl, ctype), f'{name} parameter {k} is `{decl}`, the table says {ctype}'


def test_new_symbols_overlap_no_existing_list():
    old = set(_ffi.SYMBOLS) | set(_ffi.SPILL_SYMBOLS) | set(_ffi.CUTMIG_SYMBOLS) | set(_ffi.DUALFN_SYMBOLS) | \
        set(_ffi.TREEREC_SYMBOLS) | set(_ffi.CGLP_SYMBOLS) | set(_ffi.RESTART_SYMBOLS) | set(_ffi.HEUR_SYMBOLS)
    assert not set(_ffi.PROP_SYMBOLS) & old


def test_mipx_h_includes_the_propagation_header_and_keeps_its_version():
    text = open(os.path.join(ROOT, 'include', 'mipx.h')).read()
    assert '#include "mipx_prop.h"' in text
    assert _ffi.lib().mipx_abi_version() == 1


def test_library_exports_the_propagation_entries():
    L = _ffi.lib()
    for name in _ffi.PROP_SYMBOLS:
        assert hasattr(L, name), name
        assert getattr(L, name).restype is _ffi._PROP_SIGNATURES[name][0]


def test_stats_keys_and_status_codes_cover_the_header():
    text = open(os.path.join(ROOT, 'include', 'mipx_prop.h')).read()
    assert [int(k) for k in re.findall(r'\[(\d)\] ', text)] == list(range(8))
    assert len(_ffi.PROP_STATS_KEYS) == 8 and 'tightened' in _ffi.PROP_STATS_KEYS and 'infeasible' in _ffi.PROP_STATS_KEYS
    codes = {name.lower(): int(v) for name, v in re.findall(r'#define MIPX_PROP_(\w+) (\d)', text)}
    assert codes == {v: k for k, v in _ffi.PROP_STATUS.items()}
    assert (ref.UNCHANGED, ref.TIGHTENED, ref.INFEASIBLE) == tuple(codes[k] for k in ('unchanged', 'tightened', 'infeasible'))
    assert _ffi.PROPAGATION_TOL == ref.TOL == 1e-6 and _ffi.DEFAULT_PROPAGATION_ROUNDS == 8


def test_c_entries_refuse_null_arguments():
    L = _ffi.lib()
    assert L.mipx_propagate_batch(None, 0, *([None] * 3), 0, 0.0, 1e-6, 8, *([None] * 5)) == -1   # MIPX_EINVAL
    assert L.mipx_tree_set_propagation(None, 8, 1) == -1
    assert L.mipx_tree_propagation_stats(None, None) == -1


# ---- what the constructor refuses ------------------------------------------------------------------------------
def build(**extra):
    kw = dict(pseudo_costs={}, frontier_batch=4, gomory_cuts=False, propagate=True)
    kw.update(extra)
    return BranchAndBound(model('small_branch'), PseudoCostBranchNode, **kw)


@pytest.mark.parametrize('value', [False, 0, -3, 2.5, 'on'])
def test_propagate_value(value):
    with pytest.raises(AssertionError, match='propagate is None, True or a positive number of rounds'):
        build(propagate=value)


def test_propagate_needs_frontier_batch():
    with pytest.raises(AssertionError, match='propagate needs frontier_batch'):
        build(frontier_batch=None)


def test_propagate_not_with_comm():
    with pytest.raises(AssertionError, match='propagate cannot be combined with comm'):
        build(comm=object())


def test_propagate_needs_no_cut_rounds():
    with pytest.raises(AssertionError, match='propagate needs gomory_cuts=False'):
        build(gomory_cuts=True)
    with pytest.raises(AssertionError, match='propagate needs gomory_cuts=False'):
        BranchAndBound(model('small_branch'), PseudoCostBranchNode, pseudo_costs={}, frontier_batch=4, propagate=True)


def test_propagate_not_with_the_records():
    with pytest.raises(AssertionError, match='propagate cannot be combined with dual_function'):
        build(dual_function=True)
    with pytest.raises(AssertionError, match='propagate cannot be combined with tree_record'):
        build(tree_record=True)


def test_option_is_off_by_default():
    assert build()._propagate is True and build(propagate=3)._propagate == 3 and build().propagation_stats is None
    plain = build(propagate=None)
    assert plain._propagate is None and plain.propagation_stats is None
    assert build(primal_heuristic=True, host_spill=1 << 24, dive=8)._propagate is True   # (what it works beside)


# ---- the restatement against brute force -------------------------------------------------------------------------
def test_restatement_is_valid_by_brute_force():
    """Six columns with bounds 0..3: all 4 096 points.  Over random boxes and three cutoffs no integer-feasible
    point of the box with c . x <= cutoff leaves the propagated box, and a box is called infeasible only where there
    is none."""
    rng = np.random.default_rng(7)
    n = 6
    A = np.vstack([-rng.integers(1, 6, (3, n)), rng.integers(0, 4, (2, n))]).astype(np.float64)
    b = np.array([-22.0, -24.0, -20.0, 3.0, 4.0])
    c = -rng.integers(1, 8, n).astype(np.float64)
    P = np.array(list(itertools.product(range(4), repeat=n)), dtype=np.float64)
    rows_ok = np.all(P @ A.T >= b[None, :], axis=1)
    obj = P @ c
    assert 50 < rows_ok.sum() < 4096
    feasible_best = float(obj[rows_ok].min())
    outcomes = set()
    for trial in range(21):
        l = rng.integers(0, 3, n).astype(np.float64) * (rng.random(n) < 0.5)
        u = np.maximum(l, 3.0 - rng.integers(0, 3, n) * (rng.random(n) < 0.5))
        inside = np.all((P >= l) & (P <= u), axis=1)
        for cutoff in (np.inf, feasible_best + 6.0, feasible_best):
            keep = inside & rows_ok & (obj <= cutoff)
            for rounds in (1, 8):
                lo, up, status, changed, nrounds, capped, _ = ref.propagate_one(A, b, c, l, u, range(n), cutoff, max_rounds=rounds)
                outcomes.add(status)
                if status == ref.INFEASIBLE:
                    assert not keep.any() and np.array_equal(lo, l) and np.array_equal(up, u)
                    continue
                assert np.all((P[keep] >= lo) & (P[keep] <= up))
                assert np.all(lo >= l) and np.all(up <= u) and np.all(lo <= up) and 1 <= nrounds <= rounds
                assert (status == ref.TIGHTENED) == (changed > 0) == (not (np.array_equal(lo, l) and np.array_equal(up, u)))
                assert np.array_equal(lo, np.round(lo)) and np.array_equal(up, np.round(up))
    assert outcomes == {ref.UNCHANGED, ref.TIGHTENED, ref.INFEASIBLE}


def test_restatement_edges():
    A, b, c, l, u, ints = random_dense_milp_arrays(40, 20, seed=0)
    # the root box of a packing instance: nothing to tighten, one round
    lo, up, status, changed, rounds, capped, _ = ref.propagate_one(A, b, c, l, u, ints)
    assert (status, changed, rounds, capped) == (ref.UNCHANGED, 0, 1, 0) and np.array_equal(lo, l) and np.array_equal(up, u)
    # x0 + x1 >= 3 with x1 unbounded above: ninf = 1, only the unbounded column gets a candidate; x0 <= 2 gives x1 >= 1
    A2 = np.array([[1.0, 1.0]]); b2 = np.array([3.0])
    lo, up, status, changed, _, _, _ = ref.propagate_one(A2, b2, np.ones(2), np.zeros(2), np.array([2.0, np.inf]), [0, 1])
    assert status == ref.TIGHTENED and changed == 1 and list(lo) == [0.0, 1.0] and list(up) == [2.0, np.inf]
    # both unbounded: ninf = 2, nothing
    _, _, status, _, _, _, _ = ref.propagate_one(A2, b2, np.ones(2), np.zeros(2), np.full(2, np.inf), [0, 1])
    assert status == ref.UNCHANGED
    # a cutoff below every point: infeasible through the cutoff row alone
    _, _, status, _, _, _, _ = ref.propagate_one(A, b, c, l, u, ints, cutoff=float(c @ u) - 1.0)
    assert status == ref.INFEASIBLE
    # continuous columns are never tightened
    lo, up, status, _, _, _, _ = ref.propagate_one(A2, b2, np.ones(2), np.zeros(2), np.array([2.0, np.inf]), [0])
    assert status == ref.UNCHANGED and list(lo) == [0.0, 0.0]


# ---- the input conditions of the GPU tests -------------------------------------------------------------------------
@pytest.mark.parametrize('n,m', ref.SHAPES)
def test_the_boxes_exercise_every_outcome(n, m):
    A, b, c, l, u, ints = random_dense_milp_arrays(n, m, seed=0)
    L, U = ref.boxes(A, b, l, u)
    assert L.shape == (ref.BOXES, n) and np.all(L <= U) and np.all(L >= l) and np.all(U <= u)
    out = ref.propagate(A, b, c, L, U, ints)
    assert np.sum(out['status'] == ref.TIGHTENED) >= 3 and np.sum(out['status'] == ref.INFEASIBLE) >= 5
    if n >= 40:
        assert np.sum(out['status'] == ref.UNCHANGED) >= 5
    assert out['margin'] >= 1e-9
    cut = ref.propagate(A, b, c, L, U, ints, cutoff=ref.cutoff_for(c, U))   # (the finite cutoff of the GPU tests matters)
    assert cut['margin'] >= 1e-9 and np.sum(cut['status'] != out['status']) >= 5


def test_the_mixed_family_needs_rounds():
    deep = capped = 0
    for seed in range(4):
        A, b, c, l, u, ints = ref.mixed(20, 10, 5, seed)
        L, U = ref.boxes(A, b, l, u, seed=seed)
        deep += int(np.sum(ref.propagate(A, b, c, L, U, ints, max_rounds=50)['rounds'] >= 4))
        capped += int(np.sum(ref.propagate(A, b, c, L, U, ints, max_rounds=2)['capped']))
    assert deep >= 1 and capped >= 1


def test_nodes_of_a_search_on_the_mixed_family_reach_eight_rounds():
    """Best first, most fractional, LPs by HiGHS, the restatement in front of every LP with the incumbent as the
    cutoff: over the four seeds (as far as needed) some node runs eight rounds or more."""
    most = 0
    for seed in range(4):
        A, b, c, l, u, ints = ref.mixed(20, 10, 5, seed)
        heap, tick, primal = [(-np.inf, 0, l, u)], 1, np.inf
        while heap:
            bound, _, lo, up = heapq.heappop(heap)
            if bound >= primal - 1e-9:
                continue
            lo, up, status, _, rounds, _, _ = ref.propagate_one(A, b, c, lo, up, ints, cutoff=primal, max_rounds=50)
            most = max(most, rounds)
            if status == ref.INFEASIBLE:
                continue
            r = linprog(c, A_ub=-A, b_ub=-b, bounds=list(zip(lo, up)), method='highs-ds')
            if r.status != 0 or r.fun >= primal - 1e-9:
                continue
            frac = np.abs(r.x - np.round(r.x))
            j = int(np.argmax(frac))
            if frac[j] <= 1e-6:
                primal = float(r.fun)
                continue
            for lo2, up2 in ((lo, np.where(np.arange(20) == j, np.floor(r.x[j]), up)),
                             (np.where(np.arange(20) == j, np.ceil(r.x[j]), lo), up)):
                heapq.heappush(heap, (float(r.fun), tick, lo2, up2))
                tick += 1
        print('seed', seed, 'most rounds so far', most)
        if most >= 8:
            break
    assert most >= 8


def test_the_half_continuous_instance_is_fair():
    """A / 7 with the odd columns continuous: no rounding decision of the restatement is closer than 1e-9 to
    flipping, so the kernel, which sums the rows in another order, must give the same bounds."""
    A, b, c, l, u, ints = ref.half_continuous()
    L, U = ref.boxes(A, b, l, u)
    out = ref.propagate(A, b, c, L, U, ints)
    assert out['margin'] >= 1e-9
    assert np.sum(out['status'] == ref.TIGHTENED) >= 3 and np.sum(out['status'] == ref.INFEASIBLE) >= 5
    cont = np.setdiff1d(np.arange(A.shape[1]), ints)
    assert np.array_equal(out['l'][:, cont], L[:, cont]) and np.array_equal(out['u'][:, cont], U[:, cont])
