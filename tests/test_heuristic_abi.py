"""The primal heuristic (include/mipx_heur.h), the parts that need no GPU: the header against the ctypes table and
the exported symbols, what BranchAndBound refuses at construction, and the NumPy restatement of the algorithm
(tests/support/heuristic_reference.py) against scipy's HiGHS on the generator's instances."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from scipy.optimize import Bounds, LinearConstraint, linprog, milp

from simple_mip_solver_amd import BranchAndBound, PseudoCostBranchNode, _ffi
from simple_mip_solver_amd.generators import random_dense_milp_arrays
from tests.support import heuristic_reference as ref
from tests.support.example_models import model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ['mipx_round_repair_batch', 'mipx_tree_set_heuristic', 'mipx_tree_heuristic_stats']


def heur_prototypes():
    text = open(os.path.join(ROOT, 'include', 'mipx_heur.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    text = re.sub(r'^\s*#.*$', '', text, flags=re.M)
    found = re.findall(r'([\w ]+?[\s*]+)(mipx_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;', text)
    return {name: (ret.strip(), [p.strip() for p in args.split(',') if p.strip() not in ('', 'void')])
            for ret, name, args in found}


def test_heuristic_header_and_signature_table_agree():
    scalars = {'int': C.c_int, 'int64_t': C.c_int64, 'size_t': C.c_size_t, 'double': C.c_double, 'void': None}

    def agrees(decl, ctype):
        if '*' in decl or '[' in decl:
            return ctype in (C.c_void_p, C.c_char_p) or (isinstance(ctype, type) and issubclass(ctype, C._Pointer))
        return ctype is scalars[decl.replace('const ', '').split()[0]]

    protos = heur_prototypes()
    assert sorted(protos) == sorted(_ffi.HEUR_SYMBOLS) == sorted(NAMES)
    for name, (ret, params) in protos.items():
        restype, argtypes = _ffi._HEUR_SIGNATURES[name]
        assert agrees(ret, restype), name
        assert len(params) == len(argtypes), name
        for k, (decl, ctype) in enumerate(zip(params, argtypes)):
            assert agrees(decl, ctype), f'{name} parameter {k} is `{decl}`, the table says {ctype}'


def test_new_symbols_overlap_no_existing_list():
    old = set(_ffi.SYMBOLS) | set(_ffi.SPILL_SYMBOLS) | set(_ffi.CUTMIG_SYMBOLS) | set(_ffi.DUALFN_SYMBOLS) | \
        set(_ffi.TREEREC_SYMBOLS) | set(_ffi.CGLP_SYMBOLS) | set(_ffi.RESTART_SYMBOLS)
    assert not set(_ffi.HEUR_SYMBOLS) & old


def test_mipx_h_includes_the_heuristic_header_and_keeps_its_version():
    text = open(os.path.join(ROOT, 'include', 'mipx.h')).read()
    assert '#include "mipx_heur.h"' in text
    assert _ffi.lib().mipx_abi_version() == 1


def test_library_exports_the_heuristic_entries():
    L = _ffi.lib()
    for name in _ffi.HEUR_SYMBOLS:
        assert hasattr(L, name), name
        assert getattr(L, name).restype is _ffi._HEUR_SIGNATURES[name][0]


def test_stats_keys_and_status_codes_cover_the_header():
    text = open(os.path.join(ROOT, 'include', 'mipx_heur.h')).read()
    assert [int(k) for k in re.findall(r'\[(\d)\] ', text)] == list(range(8))
    assert len(_ffi.HEUR_STATS_KEYS) == 8 and 'incumbents' in _ffi.HEUR_STATS_KEYS
    codes = {name.lower(): int(v) for name, v in re.findall(r'#define MIPX_HEUR_(\w+) (\d)', text)}
    assert codes == {v: k for k, v in _ffi.HEUR_STATUS.items()}
    assert (ref.FEASIBLE, ref.STUCK, ref.CAPPED, ref.SKIPPED) == tuple(codes[k] for k in ('feasible', 'stuck', 'capped', 'skipped'))


def test_c_entries_refuse_null_arguments():
    L = _ffi.lib()
    assert L.mipx_round_repair_batch(None, 0, *([None] * 4), 0, 1e-9, 0, *([None] * 5)) == -1   # MIPX_EINVAL
    assert L.mipx_tree_set_heuristic(None, 32, 1, 10) == -1
    assert L.mipx_tree_heuristic_stats(None, None) == -1


# ---- what the constructor refuses ------------------------------------------------------------------------------
def build(**extra):
    kw = dict(pseudo_costs={}, frontier_batch=4, gomory_cuts=False, primal_heuristic=True)
    kw.update(extra)
    return BranchAndBound(model('small_branch'), PseudoCostBranchNode, **kw)


@pytest.mark.parametrize('value', [False, 0, -3, 2.5, 'on'])
def test_primal_heuristic_value(value):
    with pytest.raises(AssertionError, match='primal_heuristic is None, True or a positive number of points per step'):
        build(primal_heuristic=value)


def test_primal_heuristic_needs_frontier_batch():
    with pytest.raises(AssertionError, match='primal_heuristic needs frontier_batch'):
        build(frontier_batch=None)


def test_primal_heuristic_not_with_comm():
    with pytest.raises(AssertionError, match='primal_heuristic cannot be combined with comm'):
        build(comm=object())


def test_primal_heuristic_needs_no_cut_rounds():
    with pytest.raises(AssertionError, match='primal_heuristic needs gomory_cuts=False'):
        build(gomory_cuts=True)
    with pytest.raises(AssertionError, match='primal_heuristic needs gomory_cuts=False'):
        BranchAndBound(model('small_branch'), PseudoCostBranchNode, pseudo_costs={}, frontier_batch=4, primal_heuristic=True)


def test_option_is_kept_for_restart_and_off_by_default():
    assert build(primal_heuristic=7)._given['primal_heuristic'] == 7
    assert build()._given['primal_heuristic'] is True and build().heuristic_stats is None
    plain = build(primal_heuristic=None)
    assert plain._given['primal_heuristic'] is None and plain._primal_heuristic is None and plain.heuristic_stats is None
    assert 'primal_heuristic' in BranchAndBound._restart_overrides


# ---- the restatement against HiGHS ------------------------------------------------------------------------------
def root_vertex(A, b, c, l, u):
    r = linprog(c, A_ub=-A, b_ub=-b, bounds=list(zip(l, u)), method='highs-ds')
    assert r.status == 0, r.message
    return np.asarray(r.x)


@pytest.mark.parametrize('n,m', [(8, 4), (20, 10), (40, 20), (64, 32)])
@pytest.mark.parametrize('seed', range(6))
def test_restatement_from_the_root_vertex(n, m, seed):
    A, b, c, l, u, ints = random_dense_milp_arrays(n, m, seed=seed)
    x = root_vertex(A, b, c, l, u)
    xt, obj, status, moves = ref.round_repair_lift_one(A, b, c, l, u, ints, x)
    assert status == ref.FEASIBLE and sum(moves) <= m + n
    ref.certify(A, b, c, l, u, ints, xt, obj)
    h = milp(c, constraints=LinearConstraint(A, lb=b, ub=np.inf), bounds=Bounds(l, u), integrality=np.ones(n),
             options={'mip_rel_gap': 0.0})
    assert h.status == 0
    # (integer data: obj is exact; HiGHS' optimum carries its own rounding, 1e-6 relative as elsewhere in this suite)
    assert obj >= h.fun - 1e-6 * max(1.0, abs(h.fun))
    floor_point = np.floor(x + 1e-9)   # (1e-9: a vertex coordinate a rounding error below an integer counts as that integer)
    assert obj <= float(c @ floor_point)


def test_restatement_edges():
    A, b, c, l, u, ints = random_dense_milp_arrays(8, 4, seed=0)
    x = np.full(8, 9.6)
    # no move allowed: the rounded point as it is, capped because rows are violated
    xt, obj, status, moves = ref.round_repair_lift_one(A, b, c, l, u, ints, x, max_moves=0)
    assert status == ref.CAPPED and moves == (0, 0) and np.array_equal(xt, np.full(8, 10.0)) and obj == float(c @ xt)
    # the bounds clamp the rounding
    xt, _, _, _ = ref.round_repair_lift_one(A, b, c, l, u, ints, np.full(8, 12.4), max_moves=0)
    assert np.array_equal(xt, u)
    # a skipped point comes back unchanged
    Xt, obj, status, moves = ref.round_repair_lift(A, b, c, l, u, ints, np.stack([x, x]), skip=[1, 0])
    assert status[0] == ref.SKIPPED and np.array_equal(Xt[0], x) and obj[0] == 0 and not moves[0].any() and status[1] != ref.SKIPPED
    # x0 + x1 >= 1.5 and -x0 - x1 >= -1.5 with integer columns: every unit move trades one violation for the other
    A2 = np.array([[1.0, 1.0], [-1.0, -1.0]]); b2 = np.array([1.5, -1.5])
    xt, _, status, moves = ref.round_repair_lift_one(A2, b2, np.array([1.0, 1.0]), np.zeros(2), np.full(2, 5.0), [0, 1],
                                                     np.array([0.6, 0.2]))
    assert status == ref.STUCK and moves == (0, 0) and np.array_equal(xt, [1.0, 0.0])
