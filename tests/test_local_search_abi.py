"""The pair-move local search (include/mipx_lsearch.h), the parts that need no GPU: the header against the ctypes table
and the exported symbols, what BranchAndBound refuses at construction, and the NumPy restatement of the algorithm
(tests/support/local_search_reference.py) against brute force and against HiGHS' optimum."""
import itertools
import os
import re

import numpy as np
import pytest
from scipy.optimize import Bounds, LinearConstraint, linprog, milp

from simple_mip_solver_amd import BranchAndBound, PseudoCostBranchNode, _ffi
from simple_mip_solver_amd.generators import random_dense_milp_arrays
from tests.support import heuristic_reference as heur
from tests.support import local_search_reference as ref
from tests.support.abi_check import agrees, prototypes
from tests.support.example_models import model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ['mipx_pair_search_batch', 'mipx_tree_set_local_search', 'mipx_tree_local_search_stats']
TOL = 1e-9


def test_local_search_header_and_signature_table_agree():
    protos = prototypes('mipx_lsearch.h')
    assert sorted(protos) == sorted(_ffi.LSEARCH_SYMBOLS) == sorted(NAMES)
    for name, (ret, params) in protos.items():
        restype, argtypes = _ffi._LSEARCH_SIGNATURES[name]
        assert agrees(ret, restype), name
        assert len(params) == len(argtypes), name
        for k, (decl, ctype) in enumerate(zip(params, argtypes)):
            assert agrees(decl, ctype), f'{name} parameter {k} is `{decl}`, the table says {ctype}'


def test_new_symbols_overlap_no_existing_list():
    old = set(_ffi.SYMBOLS) | set(_ffi.SPILL_SYMBOLS) | set(_ffi.CUTMIG_SYMBOLS) | set(_ffi.DUALFN_SYMBOLS) | \
        set(_ffi.TREEREC_SYMBOLS) | set(_ffi.CGLP_SYMBOLS) | set(_ffi.RESTART_SYMBOLS) | set(_ffi.HEUR_SYMBOLS) | \
        set(_ffi.PROP_SYMBOLS) | set(_ffi.RCFIX_SYMBOLS) | set(_ffi.OBJSTEP_SYMBOLS)
    assert not set(_ffi.LSEARCH_SYMBOLS) & old


def test_mipx_h_includes_the_local_search_header_and_keeps_its_version():
    text = open(os.path.join(ROOT, 'include', 'mipx.h')).read()
    assert '#include "mipx_lsearch.h"' in text
    assert _ffi.lib().mipx_abi_version() == 1


def test_library_exports_the_local_search_entries():
    L = _ffi.lib()
    for name in _ffi.LSEARCH_SYMBOLS:
        assert hasattr(L, name), name
        assert getattr(L, name).restype is _ffi._LSEARCH_SIGNATURES[name][0]


def test_stats_keys_and_status_codes_cover_the_header():
    text = open(os.path.join(ROOT, 'include', 'mipx_lsearch.h')).read()
    assert [int(k) for k in re.findall(r'\[(\d)\] ', text)] == list(range(8))
    assert len(_ffi.LSEARCH_STATS_KEYS) == 8 and len(set(_ffi.LSEARCH_STATS_KEYS)) == 8
    assert _ffi.LSEARCH_STATS_KEYS == ('points', 'improved', 'single_moves', 'pair_moves', 'capped', 'incumbents', 'reserved',
                                       'kernel_us')
    codes = {name.lower(): int(v) for name, v in re.findall(r'#define MIPX_LS_(\w+) (\d)', text)}
    assert codes == {v: k for k, v in _ffi.LSEARCH_STATUS.items()} and len(codes) == 4
    assert (ref.LOCAL_OPT, ref.CAPPED, ref.NOT_FEASIBLE, ref.SKIPPED) == \
        tuple(codes[k] for k in ('local_opt', 'capped', 'not_feasible', 'skipped'))
    assert _ffi.DEFAULT_LOCAL_SEARCH_MOVES == 64


def test_c_entries_refuse_null_arguments():
    L = _ffi.lib()
    assert L.mipx_pair_search_batch(None, 0, *([None] * 4), 0, 1e-9, 4, *([None] * 5)) == -1   # MIPX_EINVAL
    assert L.mipx_tree_set_local_search(None, 4) == -1
    assert L.mipx_tree_local_search_stats(None, None) == -1


# ---- what the constructor refuses ------------------------------------------------------------------------------
def build(**extra):
    kw = dict(pseudo_costs={}, frontier_batch=4, gomory_cuts=False, primal_heuristic=True, local_search=True)
    kw.update(extra)
    return BranchAndBound(model('small_branch'), PseudoCostBranchNode, **kw)


@pytest.mark.parametrize('value', [False, 0, -3, 2.5, 'on'])
def test_local_search_value(value):
    with pytest.raises(AssertionError, match='local_search is None, True or a positive number of moves'):
        build(local_search=value)


def test_local_search_needs_the_heuristic():
    with pytest.raises(AssertionError, match='local_search needs primal_heuristic'):
        build(primal_heuristic=None)
    with pytest.raises(AssertionError, match='primal_heuristic needs frontier_batch'):   # (and so frontier_batch and no cut rounds)
        build(frontier_batch=None)
    with pytest.raises(AssertionError, match='primal_heuristic needs gomory_cuts=False'):
        build(gomory_cuts=True)
    with pytest.raises(AssertionError, match='primal_heuristic cannot be combined with comm'):
        build(comm=object())


def test_option_is_off_by_default_and_inherited_by_restart():
    on = build()
    assert on._local_search is True and on.local_search_stats is None and on._given['local_search'] is True
    assert build(local_search=7)._given['local_search'] == 7
    plain = build(local_search=None)
    assert plain._local_search is None and plain._given['local_search'] is None and plain.local_search_stats is None
    assert 'local_search' in BranchAndBound._restart_overrides and 'primal_heuristic' in BranchAndBound._restart_overrides
    # (what it works beside)
    assert build(propagate=True, reduced_cost=True, objective_step=True, host_spill=1 << 24, dive=8, anchor=False)._local_search is True
    assert build(tree_record=True)._local_search is True and build(dual_function=True)._local_search is True


def test_restart_without_the_heuristic_drops_the_local_search(monkeypatch):
    """restart(primal_heuristic=None) on a search with local_search: the new search has neither (the constructor is
    reached with local_search=None, not with an assertion about an option the caller never named); an explicit
    local_search beside it is the caller's and is refused as the constructor refuses it."""
    from simple_mip_solver_amd.lp import CyLPArray
    src = build(tree_record=True)
    src.status = 'optimal'
    seeded = []
    monkeypatch.setattr(BranchAndBound, '_seed_native', lambda self, source: seeded.append(self))
    b = CyLPArray(np.asarray(src.root_node.lp.constraints[0].lower, dtype=np.float64).copy())
    new = src.restart(b, primal_heuristic=None)
    assert new._primal_heuristic is None and new._local_search is None and seeded == [new]
    kept = src.restart(b)
    assert kept._primal_heuristic is True and kept._local_search is True
    fewer = src.restart(b, local_search=3)
    assert fewer._local_search == 3 and fewer._primal_heuristic is True
    with pytest.raises(AssertionError, match='local_search needs primal_heuristic'):
        src.restart(b, primal_heuristic=None, local_search=True)


# ---- the restatement against brute force -------------------------------------------------------------------------
def feasible(A, b, x):
    return bool(np.all(A @ x - b >= -TOL))


def neighbours(x, ints, lo, hi):
    """Every single and every pair move of x inside the bounds, by enumeration."""
    moves = [((j, d),) for j in ints for d in (1.0, -1.0)]
    moves += [((j, dj), (k, dk)) for j, k in itertools.combinations(sorted(ints), 2) for dj in (1.0, -1.0) for dk in (1.0, -1.0)]
    for mv in moves:
        y = x.copy()
        for j, d in mv:
            y[j] += d
        if all(lo[j] <= y[j] <= hi[j] for j, _ in mv):
            yield mv, y


def best_neighbour(A, b, c, x, ints, lo, hi):
    """The smallest key (g, j, k, dj, dk) among the feasible improving neighbours, or None -- by enumeration, on
    dyadic data (every sum exact)."""
    best = None
    for mv, y in neighbours(x, ints, lo, hi):
        g = sum(c[j] * d for j, d in mv)
        if g < 0 and feasible(A, b, y):
            (j, dj), (k, dk) = mv[0], (mv[1] if len(mv) > 1 else (-1, 0.0))
            key = (g, j, k, 0 if dj > 0 else 1, 0 if dk >= 0 else 1)
            if best is None or key < best[0]:
                best = (key, y)
    return best


def small_problem(rng, mixed):
    """n <= 6 columns, bounds inside 0..3, a feasible integral start.  mixed: packing and covering rows and the last
    column continuous (its value a multiple of 1/4: every sum stays exact)."""
    n, m = int(rng.integers(2 if mixed else 1, 7)), int(rng.integers(1, 5))
    if mixed:
        A = rng.integers(0, 5, (m, n)).astype(np.float64) * np.where(rng.random(m) < 0.5, 1.0, -1.0)[:, None]
    else:
        A = rng.integers(-4, 5, (m, n)).astype(np.float64)
    c = rng.integers(-6, 7, n).astype(np.float64)
    l = rng.integers(0, 2, n).astype(np.float64)
    u = np.minimum(3.0, l + rng.integers(0, 4, n))
    x = np.floor(l + rng.random(n) * (u - l + 1))
    ints = list(range(n))
    if mixed:
        ints = ints[:-1]
        x[-1] = l[-1] + 0.25 * rng.integers(0, 4 * int(u[-1] - l[-1]) + 1)
    b = A @ x - rng.integers(0, 4, m)
    return A, b, c, l, u, ints, x


@pytest.mark.parametrize('mixed', [False, True], ids=['integer', 'mixed'])
def test_restatement_by_brute_force(mixed):
    rng = np.random.default_rng(23 + mixed)
    outcomes, moved, pair_moves = set(), 0, 0
    for trial in range(250):
        A, b, c, l, u, ints, x = small_problem(rng, mixed)
        assert feasible(A, b, x)
        cont = np.setdiff1d(np.arange(len(x)), ints)
        for cap in (64, int(rng.integers(0, 3))):
            xo, obj, status, (singles, pairs) = ref.pair_search_one(A, b, c, l, u, ints, x, tol=TOL, max_moves=cap)
            outcomes.add(status)
            assert status in (ref.LOCAL_OPT, ref.CAPPED)
            # feasible, integral, inside the bounds, continuous columns untouched, no worse, obj = c . x
            assert feasible(A, b, xo) and np.array_equal(xo[ints], np.round(xo[ints]))
            assert np.all(xo >= l) and np.all(xo <= u) and np.array_equal(xo[cont], x[cont])
            assert obj == float(c @ xo) <= float(c @ x)
            assert (singles + pairs > 0) == (obj < float(c @ x))
            if status == ref.LOCAL_OPT:   # no neighbour is both feasible and improving
                assert best_neighbour(A, b, c, xo, ints, l, u) is None
                assert singles + pairs <= cap
            else:                         # exactly the cap, and a move remains
                assert singles + pairs == cap and best_neighbour(A, b, c, xo, ints, l, u) is not None
            moved += singles + pairs
            pair_moves += pairs
        # move by move: each move is the smallest key of the enumeration
        y, steps = x.copy(), 0
        while True:
            nb = best_neighbour(A, b, c, y, ints, l, u)
            got = ref.pair_search_one(A, b, c, l, u, ints, y, tol=TOL, max_moves=1)
            if nb is None:
                assert got[2] == ref.LOCAL_OPT and got[3] == (0, 0) and np.array_equal(got[0], y)
                break
            assert np.array_equal(got[0], nb[1]) and got[3] == ((1, 0) if nb[0][2] < 0 else (0, 1))
            y, steps = nb[1], steps + 1
        full = ref.pair_search_one(A, b, c, l, u, ints, x, tol=TOL, max_moves=64)
        assert np.array_equal(full[0], y) and sum(full[3]) == steps
    print(outcomes, moved, pair_moves)
    assert outcomes == {ref.LOCAL_OPT, ref.CAPPED} and moved > 200 and pair_moves > 50


def test_restatement_returns_bad_points_unchanged():
    rng = np.random.default_rng(5)
    seen = 0
    for trial in range(100):
        A, b, c, l, u, ints, x = small_problem(rng, trial % 2 == 1)
        j = ints[int(rng.integers(len(ints)))]
        for what, bad, rows in (('fractional', x + 0.5 * (np.arange(len(x)) == j), b), ('above', x + (u[j] + 1 - x[j]) * (np.arange(len(x)) == j), b),
                                ('below', x - (x[j] - l[j] + 1) * (np.arange(len(x)) == j), b), ('row', x, b + 4.0 + np.abs(A).sum(axis=1))):
            if what == 'row' and not np.any(A @ x - rows < -TOL):
                continue
            xo, obj, status, moves = ref.pair_search_one(A, rows, c, l, u, ints, bad, tol=TOL)
            assert status == ref.NOT_FEASIBLE and moves == (0, 0) and np.array_equal(xo, bad) and obj == float(c @ bad), what
            seen += 1
    assert seen >= 300
    # the batch: a skipped point comes back unchanged with obj 0
    A, b, c, l, u, ints, x = small_problem(np.random.default_rng(1), False)
    Xo, obj, status, moves = ref.pair_search(A, b, c, l, u, ints, np.stack([x, x]), skip=[1, 0])
    assert status[0] == ref.SKIPPED and obj[0] == 0.0 and np.array_equal(Xo[0], x) and not moves[0].any() and status[1] != ref.SKIPPED


def test_restatement_edges():
    # max x0 + x1 with x0 + x1 <= 3, from (0, 0): one pair move, then a single, then nothing
    A = np.array([[-1.0, -1.0]]); b = np.array([-3.0]); c = np.array([-1.0, -1.0]); l = np.zeros(2); u = np.full(2, 5.0)
    xo, obj, status, moves = ref.pair_search_one(A, b, c, l, u, [0, 1], [0.0, 0.0])
    assert list(xo) == [2.0, 1.0] and obj == -3.0 and status == ref.LOCAL_OPT and moves == (1, 1)   # (ties: the lower column)
    # a swap: max 3 x0 + x1 with x0 + x1 <= 2 from (0, 2): (x0 + 1, x1 - 1) twice, no single fits
    c = np.array([-3.0, -1.0]); b = np.array([-2.0])
    xo, obj, status, moves = ref.pair_search_one(A, b, c, l, u, [0, 1], [0.0, 2.0])
    assert list(xo) == [2.0, 0.0] and obj == -6.0 and moves == (0, 2)
    assert ref.pair_search_one(A, b, c, l, u, [0, 1], [0.0, 2.0], max_moves=1)[2:] == (ref.CAPPED, (0, 1))
    assert ref.pair_search_one(A, b, c, l, u, [0, 1], [0.0, 2.0], max_moves=2)[2:] == (ref.LOCAL_OPT, (0, 2))
    assert ref.pair_search_one(A, b, c, l, u, [0, 1], [0.0, 2.0], max_moves=0)[2:] == (ref.CAPPED, (0, 0))
    # only integer columns move; the rounded bounds hold
    assert list(ref.pair_search_one(A, b, c, l, u, [1], [0.0, 2.0])[0]) == [0.0, 2.0]
    assert list(ref.pair_search_one(A, b, c, l, [1.75, 5.0], [0, 1], [0.0, 2.0])[0]) == [1.0, 1.0]
    # no columns at all to move, no rows
    assert ref.pair_search_one(np.zeros((0, 2)), np.zeros(0), c, l, u, [], [0.5, 0.5])[2:] == (ref.LOCAL_OPT, (0, 0))
    assert list(ref.pair_search_one(np.zeros((0, 2)), np.zeros(0), c, l, u, [0, 1], [0.0, 0.0])[0]) == [5.0, 5.0]


@pytest.mark.parametrize('seed', range(6))
@pytest.mark.parametrize('n,m', [(8, 4), (16, 8), (32, 16), (64, 32)])
def test_restatement_never_goes_below_the_optimum(n, m, seed):
    """From the heuristic's point at the root LP vertex: the search ends feasible at a local optimum, no worse than it
    began and never below HiGHS' optimum."""
    A, b, c, l, u, ints = random_dense_milp_arrays(n, m, seed=seed)
    r = linprog(c, A_ub=-A, b_ub=-b, bounds=list(zip(l, u)), method='highs-ds')
    h = milp(c, constraints=LinearConstraint(A, lb=b, ub=np.inf), bounds=Bounds(l, u), integrality=np.ones(n),
             options={'mip_rel_gap': 0.0})
    assert r.status == 0 and h.status == 0
    xt, obj0, status, _ = heur.round_repair_lift_one(A, b, c, l, u, ints, r.x)
    assert status == heur.FEASIBLE
    xo, obj, status, moves = ref.pair_search_one(A, b, c, l, u, ints, xt)
    print(n, m, seed, 'heuristic', obj0, 'search', obj, moves, 'optimum', h.fun)
    assert status == ref.LOCAL_OPT
    heur.certify(A, b, c, l, u, ints, xo, obj)
    assert float(h.fun) - 1e-6 <= obj <= obj0
