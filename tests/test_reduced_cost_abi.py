"""The reduced-cost bound tightening (include/mipx_rcfix.h), the parts that need no GPU: the header against the ctypes
table and the exported symbols, what BranchAndBound refuses at construction, the NumPy restatement of the algorithm
(tests/support/reduced_cost_reference.py) against brute force, and the input conditions of the GPU tests."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from simple_mip_solver_amd import BranchAndBound, PseudoCostBranchNode, _ffi
from simple_mip_solver_amd.generators import random_dense_milp_arrays
from tests.support import propagation_reference as prop_ref
from tests.support import reduced_cost_reference as ref
from tests.support.example_models import model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ['mipx_reduced_cost_tighten_batch', 'mipx_tree_set_reduced_cost', 'mipx_tree_reduced_cost_stats']


def rcfix_prototypes():
    text = open(os.path.join(ROOT, 'include', 'mipx_rcfix.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    text = re.sub(r'^\s*#.*$', '', text, flags=re.M)
    found = re.findall(r'([\w ]+?[\s*]+)(mipx_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;', text)
    return {name: (ret.strip(), [p.strip() for p in args.split(',') if p.strip() not in ('', 'void')])
            for ret, name, args in found}


def test_reduced_cost_header_and_signature_table_agree():
    scalars = {'int': C.c_int, 'int64_t': C.c_int64, 'size_t': C.c_size_t, 'double': C.c_double, 'void': None}

    def agrees(decl, ctype):
        if '*' in decl or '[' in decl:
            return ctype in (C.c_void_p, C.c_char_p) or (isinstance(ctype, type) and issubclass(ctype, C._Pointer))
        return ctype is scalars[decl.replace('const ', '').split()[0]]

    protos = rcfix_prototypes()
    assert sorted(protos) == sorted(_ffi.RCFIX_SYMBOLS) == sorted(NAMES)
    for name, (ret, params) in protos.items():
        restype, argtypes = _ffi._RCFIX_SIGNATURES[name]
        assert agrees(ret, restype), name
        assert len(params) == len(argtypes), name
        for k, (decl, ctype) in enumerate(zip(params, argtypes)):
            assert agrees(decl, ctype), f'{name} parameter {k} is `{decl}`, the table says {ctype}'


def test_new_symbols_overlap_no_existing_list():
    old = set(_ffi.SYMBOLS) | set(_ffi.SPILL_SYMBOLS) | set(_ffi.CUTMIG_SYMBOLS) | set(_ffi.DUALFN_SYMBOLS) | \
        set(_ffi.TREEREC_SYMBOLS) | set(_ffi.CGLP_SYMBOLS) | set(_ffi.RESTART_SYMBOLS) | set(_ffi.HEUR_SYMBOLS) | \
        set(_ffi.PROP_SYMBOLS)
    assert not set(_ffi.RCFIX_SYMBOLS) & old


def test_mipx_h_includes_the_reduced_cost_header_and_keeps_its_version():
    text = open(os.path.join(ROOT, 'include', 'mipx.h')).read()
    assert '#include "mipx_rcfix.h"' in text
    assert _ffi.lib().mipx_abi_version() == 1


def test_library_exports_the_reduced_cost_entries():
    L = _ffi.lib()
    for name in _ffi.RCFIX_SYMBOLS:
        assert hasattr(L, name), name
        assert getattr(L, name).restype is _ffi._RCFIX_SIGNATURES[name][0]


def test_stats_keys_and_status_codes_cover_the_header():
    text = open(os.path.join(ROOT, 'include', 'mipx_rcfix.h')).read()
    assert [int(k) for k in re.findall(r'\[(\d)\] ', text)] == list(range(8))
    assert len(_ffi.RCFIX_STATS_KEYS) == 8 and len(set(_ffi.RCFIX_STATS_KEYS)) == 8
    assert _ffi.RCFIX_STATS_KEYS[:6] == ('nodes', 'tightened', 'cut_off', 'no_bound', 'bounds_changed', 'launches')
    assert _ffi.RCFIX_STATS_KEYS[6:] == ('reserved', 'kernel_us')
    codes = {name.lower(): int(v) for name, v in re.findall(r'#define MIPX_RCFIX_(\w+) (\d)', text)}
    assert codes == {v: k for k, v in _ffi.RCFIX_STATUS.items()} and len(codes) == 4
    assert (ref.UNCHANGED, ref.TIGHTENED, ref.CUT_OFF, ref.NO_BOUND) == \
        tuple(codes[k] for k in ('unchanged', 'tightened', 'cut_off', 'no_bound'))
    assert _ffi.RCFIX_TOL == ref.TOL == 1e-6 and _ffi.RCFIX_DTOL == ref.DTOL == 1e-9


def test_c_entries_refuse_null_arguments():
    L = _ffi.lib()
    assert L.mipx_reduced_cost_tighten_batch(None, 0, *([None] * 4), 0, 0.0, 1e-6, 1e-9, *([None] * 5)) == -1   # MIPX_EINVAL
    assert L.mipx_tree_set_reduced_cost(None, 1) == -1
    assert L.mipx_tree_reduced_cost_stats(None, None) == -1


# ---- what the constructor refuses ------------------------------------------------------------------------------
def build(**extra):
    kw = dict(pseudo_costs={}, frontier_batch=4, gomory_cuts=False, reduced_cost=True)
    kw.update(extra)
    return BranchAndBound(model('small_branch'), PseudoCostBranchNode, **kw)


@pytest.mark.parametrize('value', [False, 0, 1, 3, 2.5, 'on'])
def test_reduced_cost_value(value):
    with pytest.raises(AssertionError, match='reduced_cost is None or True'):
        build(reduced_cost=value)


def test_reduced_cost_needs_frontier_batch():
    with pytest.raises(AssertionError, match='reduced_cost needs frontier_batch'):
        build(frontier_batch=None)


def test_reduced_cost_not_with_comm():
    with pytest.raises(AssertionError, match='reduced_cost cannot be combined with comm'):
        build(comm=object())


def test_reduced_cost_needs_no_cut_rounds():
    with pytest.raises(AssertionError, match='reduced_cost needs gomory_cuts=False'):
        build(gomory_cuts=True)
    with pytest.raises(AssertionError, match='reduced_cost needs gomory_cuts=False'):
        BranchAndBound(model('small_branch'), PseudoCostBranchNode, pseudo_costs={}, frontier_batch=4, reduced_cost=True)


def test_reduced_cost_not_with_the_records_nor_with_restart():
    with pytest.raises(AssertionError, match='reduced_cost cannot be combined with dual_function'):
        build(dual_function=True)
    with pytest.raises(AssertionError, match='reduced_cost cannot be combined with tree_record'):
        build(tree_record=True)
    with pytest.raises(AssertionError, match='restart needs a search run with frontier_batch and tree_record=True'):
        build().restart(None)
    with pytest.raises(AssertionError, match='restart overrides are'):   # (nor can a restart turn it on)
        bb = build(reduced_cost=None, tree_record=True)
        bb.status = 'optimal'
        bb.restart(None, reduced_cost=True)


def test_option_is_off_by_default():
    assert build()._reduced_cost is True and build().reduced_cost_stats is None
    plain = build(reduced_cost=None)
    assert plain._reduced_cost is None and plain.reduced_cost_stats is None
    # (what it works beside)
    assert build(primal_heuristic=True, propagate=True, host_spill=1 << 24, dive=8, anchor=False)._reduced_cost is True


# ---- the restatement against brute force -------------------------------------------------------------------------
def test_restatement_is_valid_by_brute_force():
    """n <= 6, m <= 4, boxes inside [0, 3]^n, random y with negative and NaN entries, random cutoffs: every integer
    point of the box with A x >= b and c . x <= U lies in the output box, and CUT_OFF implies there is none."""
    rng = np.random.default_rng(11)
    outcomes, moved, points = set(), 0, 0
    for trial in range(300):
        n, m = int(rng.integers(1, 7)), int(rng.integers(1, 5))
        A = rng.integers(-4, 5, (m, n)).astype(np.float64)
        c = rng.integers(-6, 7, n).astype(np.float64)
        l = rng.integers(0, 3, n).astype(np.float64)
        u = np.minimum(3.0, l + rng.integers(0, 4, n))
        x0 = np.floor(l + rng.random(n) * (u - l + 1))          # a point of the box: most trials have feasible points
        b = A @ x0 - rng.integers(0, 4, m)
        y = rng.normal(0.0, 1.5, m) * (rng.random(m) < 0.8)
        y[rng.random(m) < 0.1] = np.nan
        ints = np.flatnonzero(rng.random(n) < 0.8)
        for cutoff in (float(c @ x0) + float(rng.integers(-3, 6)), float(c @ x0) + rng.random(), np.inf):
            lo, up, z, status, changed = ref.tighten_one(A, b, c, l, u, y, ints, cutoff)
            outcomes.add(status)
            points += ref.brute_force_check(A, b, c, l, u, cutoff, lo, up, status)
            assert (status == ref.TIGHTENED) == (changed > 0) == (not (np.array_equal(lo, l) and np.array_equal(up, u)))
            cont = np.setdiff1d(np.arange(n), ints)
            assert np.array_equal(lo[cont], l[cont]) and np.array_equal(up[cont], u[cont])
            assert np.array_equal(lo, np.round(lo)) and np.array_equal(up, np.round(up))
            assert (status == ref.NO_BOUND) == (not np.isfinite(cutoff))
            moved += changed
    print(outcomes, moved, points)
    assert outcomes == {ref.UNCHANGED, ref.TIGHTENED, ref.CUT_OFF, ref.NO_BOUND} and moved > 100 and points > 1000


def test_restatement_with_lp_duals_keeps_the_optimum():
    """The duals of the root LP and the optimum as the cutoff (the CPU simulation's root case): many columns of a
    packing instance get a tighter bound, and the optimal point stays inside."""
    from scipy.optimize import Bounds, LinearConstraint, milp
    A, b, c, l, u, ints = random_dense_milp_arrays(40, 20, seed=0)
    Y, ok = ref.highs_duals(A, b, c, l[None, :], u[None, :])
    h = milp(c, constraints=LinearConstraint(A, lb=b, ub=np.inf), bounds=Bounds(l, u), integrality=np.ones(len(c)),
             options={'mip_rel_gap': 0.0})
    assert ok[0] and h.status == 0
    lo, up, z, status, changed = ref.tighten_one(A, b, c, l, u, Y[0], ints, float(h.fun))
    x = np.round(h.x)
    print(changed, z, h.fun)
    assert status == ref.TIGHTENED and changed >= 20 and z <= h.fun + 1e-9
    assert np.all(x >= lo) and np.all(x <= up)


def test_restatement_edges():
    A = np.array([[1.0, 1.0]]); b = np.array([2.0]); c = np.array([1.0, -1.0])
    # y = 0: d = c, z = c . (l, u) = 0 * 1 - 1 * 3 = -3; cutoff -1: g = 2, x0 <= 0 + 2, x1 >= 3 - 2
    lo, up, z, status, changed = ref.tighten_one(A, b, c, [0, 0], [5, 3], [0.0], [0, 1], -1.0)
    assert (z, status, changed) == (-3.0, ref.TIGHTENED, 2) and list(lo) == [0.0, 1.0] and list(up) == [2.0, 3.0]
    # only integer columns move
    lo, up, z, status, changed = ref.tighten_one(A, b, c, [0, 0], [5, 3], [0.0], [1], -1.0)
    assert (status, changed) == (ref.TIGHTENED, 1) and list(lo) == [0.0, 1.0] and list(up) == [5.0, 3.0]
    # u = +inf under d < 0: z = -inf, no bound; an infinite cutoff: no bound
    assert ref.tighten_one(A, b, c, [0, 0], [5, np.inf], [0.0], [0, 1], -1.0)[2:] == (-np.inf, ref.NO_BOUND, 0)
    assert ref.tighten_one(A, b, c, [0, 0], [5, 3], [0.0], [0, 1], np.inf)[3] == ref.NO_BOUND
    # u = +inf under d > 0 is tightened: y = 2 gives d = (-1, -3), y = 0.5 gives d = (0.5, -1.5)
    lo, up, z, status, changed = ref.tighten_one(A, b, c, [0, 0], [np.inf, 3], [0.5], [0, 1], -1.0)
    assert z == 0.5 * 2.0 - 1.5 * 3.0 and status == ref.TIGHTENED and up[0] == np.floor(2.5 / 0.5 + 1e-6)
    # a cutoff below z by more than the slack: cut off; within the slack: g = 0 fixes the columns at their bounds
    assert ref.tighten_one(A, b, c, [0, 0], [5, 3], [0.0], [0, 1], -3.5)[3] == ref.CUT_OFF
    lo, up, z, status, changed = ref.tighten_one(A, b, c, [0, 0], [5, 3], [0.0], [0, 1], -3.0 - 5e-7)
    assert status == ref.TIGHTENED and list(lo) == [0.0, 3.0] and list(up) == [0.0, 3.0]
    # negative and NaN duals count as 0
    for y in ([-4.0], [np.nan]):
        assert ref.tighten_one(A, b, c, [0, 0], [5, 3], y, [0, 1], -1.0)[2] == -3.0
    # |d| <= dtol: the column is skipped
    lo, up, z, status, changed = ref.tighten_one(A, b, np.array([1e-10, -1e-10]), [0, 0], [5, 3], [0.0], [0, 1], 0.0)
    assert status == ref.UNCHANGED
    # more columns than partial sums: the order of the header still gives the exact sum on integer data
    n = 700
    d, z = ref.bound_of(np.zeros((1, n)), np.zeros(1), np.arange(1.0, n + 1), np.ones(n), np.full(n, 2.0), np.zeros(1))
    assert z == n * (n + 1) / 2


# ---- the input conditions of the GPU tests -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def shape_case(n, m):
    A, b, c, l, u, ints = random_dense_milp_arrays(n, m, seed=0)
    L, U = prop_ref.boxes(A, b, l, u)
    count = ref.boxes_of(n, m)
    L, U = L[:count], U[:count]
    Y, feasible = ref.highs_duals(A, b, c, L, U)
    z = ref.tighten(A, b, c, L, U, Y, ints, np.inf)['z']
    return A, b, c, L, U, Y, ints, feasible, ref.cutoff_for(z, feasible)


@pytest.mark.parametrize('n,m', prop_ref.SHAPES)
def test_the_boxes_and_the_cutoff_exercise_the_outcomes(n, m):
    """With HiGHS' duals and the cutoff of the shape at least one box is tightened and at least one is cut off, and
    box 0 (the root box) is not cut off: a kernel that never tightens cannot pass the GPU comparison."""
    A, b, c, L, U, Y, ints, feasible, cutoff = shape_case(n, m)
    out = ref.tighten(A, b, c, L, U, Y, ints, cutoff)
    tightened, cut = int(np.sum(out['status'] == ref.TIGHTENED)), int(np.sum(out['status'] == ref.CUT_OFF))
    print(n, m, 'cutoff', cutoff, 'tightened', tightened, 'cut off', cut, 'feasible', int(feasible.sum()), 'of', len(L))
    assert feasible[0] and tightened >= 1 and cut >= 1 and out['status'][0] != ref.CUT_OFF
    assert np.all(out['changed'][out['status'] == ref.TIGHTENED] >= 1)
    assert np.all(np.isfinite(out['z'][feasible]))


def test_the_dyadic_duals_make_every_order_exact():
    """y in multiples of 1/8 on the generator's integer data: every d_j, t_j and partial sum is a multiple of 1/8
    far below 2^53 / 8, so any order of summation gives the bits of the stated one."""
    A, b, c, l, u, ints = random_dense_milp_arrays(300, 150, seed=0)
    L, U = prop_ref.boxes(A, b, l, u)
    for arr in (A, b, c, L, U):
        assert np.array_equal(arr, np.round(arr))
    Y = ref.dyadic_duals(150, len(L))
    out = ref.tighten(A, b, c, L, U, Y, ints, np.inf)
    d0, _ = ref.bound_of(A, b, c, L[0], U[0], Y[0])
    assert np.array_equal(d0 * 8, np.round(d0 * 8)) and np.array_equal(out['z'] * 8, np.round(out['z'] * 8))
    assert np.max(np.abs(out['z'])) < 2.0 ** 40
    # (another order: NumPy's pairwise sums)
    yp = np.where(Y[0] > 0, Y[0], 0.0)
    d_alt = c - A.T @ yp
    assert np.array_equal(d_alt, d0)
    assert float(yp @ b + np.sum(np.where(d0 > 0, d0 * L[0], d0 * U[0]))) == out['z'][0]

