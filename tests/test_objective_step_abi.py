"""The objective-step cutoff (include/mipx_objstep.h), the parts that need no GPU: the header against the ctypes table
and the exported symbols, what BranchAndBound refuses at construction, and objective_step_of."""
import os
import re

import numpy as np
import pytest

from simple_mip_solver_amd import BranchAndBound, MILPInstance, PseudoCostBranchNode, _ffi
from simple_mip_solver_amd.generators import random_dense_milp_arrays
from simple_mip_solver_amd.utils.objective_step import objective_step_of
from tests.support.abi_check import agrees, prototypes
from tests.support.example_models import model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ['mipx_tree_set_objective_step', 'mipx_tree_objective_step_stats']


def test_objective_step_header_and_signature_table_agree():
    protos = prototypes('mipx_objstep.h')
    assert sorted(protos) == sorted(_ffi.OBJSTEP_SYMBOLS) == sorted(NAMES)
    for name, (ret, params) in protos.items():
        restype, argtypes = _ffi._OBJSTEP_SIGNATURES[name]
        assert agrees(ret, restype), name
        assert len(params) == len(argtypes), name
        for k, (decl, ctype) in enumerate(zip(params, argtypes)):
            assert agrees(decl, ctype), f'{name} parameter {k} is `{decl}`, the table says {ctype}'


def test_new_symbols_overlap_no_existing_list():
    old = set(_ffi.SYMBOLS) | set(_ffi.SPILL_SYMBOLS) | set(_ffi.CUTMIG_SYMBOLS) | set(_ffi.DUALFN_SYMBOLS) | \
        set(_ffi.TREEREC_SYMBOLS) | set(_ffi.CGLP_SYMBOLS) | set(_ffi.RESTART_SYMBOLS) | set(_ffi.HEUR_SYMBOLS) | \
        set(_ffi.PROP_SYMBOLS) | set(_ffi.RCFIX_SYMBOLS) | set(_ffi.LSEARCH_SYMBOLS)
    assert not set(_ffi.OBJSTEP_SYMBOLS) & old


def test_mipx_h_includes_the_objective_step_header_and_keeps_its_version():
    text = open(os.path.join(ROOT, 'include', 'mipx.h')).read()
    assert '#include "mipx_objstep.h"' in text
    assert _ffi.lib().mipx_abi_version() == 1


def test_library_exports_the_objective_step_entries():
    L = _ffi.lib()
    for name in _ffi.OBJSTEP_SYMBOLS:
        assert hasattr(L, name), name
        assert getattr(L, name).restype is _ffi._OBJSTEP_SIGNATURES[name][0]


def test_stats_keys_cover_the_header():
    text = open(os.path.join(ROOT, 'include', 'mipx_objstep.h')).read()
    assert [int(k) for k in re.findall(r'\[(\d)\] ', text)] == list(range(8))
    assert len(_ffi.OBJSTEP_STATS_KEYS) == 8 and len(set(_ffi.OBJSTEP_STATS_KEYS)) == 8
    assert _ffi.OBJSTEP_STATS_KEYS[:3] == ('closed_at_pop', 'left_unbranched', 'launches')
    assert all(k.startswith('reserved') for k in _ffi.OBJSTEP_STATS_KEYS[3:])
    # the header says what the caller guarantees, and what that asks of a bound handed in
    flat = ' '.join(text.split())
    assert 'differ by a multiple of step' in flat and 'mipx_tree_set_primal_bound must then be the objective of a feasible point' in flat


def test_c_entries_refuse_null_arguments():
    L = _ffi.lib()
    assert L.mipx_tree_set_objective_step(None, 1.0) == -1   # MIPX_EINVAL
    assert L.mipx_tree_objective_step_stats(None, None) == -1


# ---- what the constructor refuses ------------------------------------------------------------------------------
def build(**extra):
    kw = dict(pseudo_costs={}, frontier_batch=4, gomory_cuts=False, objective_step=True)
    kw.update(extra)
    return BranchAndBound(model('small_branch'), PseudoCostBranchNode, **kw)


@pytest.mark.parametrize('value', [False, 0, 0.0, -1, -0.5, float('inf'), float('nan'), 'on'])
def test_objective_step_value(value):
    with pytest.raises(AssertionError, match='objective_step is None, True or a positive finite step'):
        build(objective_step=value)


def test_objective_step_needs_frontier_batch():
    with pytest.raises(AssertionError, match='objective_step needs frontier_batch'):
        build(frontier_batch=None)


def test_objective_step_not_with_comm():
    with pytest.raises(AssertionError, match='objective_step cannot be combined with comm'):
        build(comm=object())


def test_objective_step_needs_no_cut_rounds():
    with pytest.raises(AssertionError, match='objective_step needs gomory_cuts=False'):
        build(gomory_cuts=True)
    with pytest.raises(AssertionError, match='objective_step needs gomory_cuts=False'):
        BranchAndBound(model('small_branch'), PseudoCostBranchNode, pseudo_costs={}, frontier_batch=4, objective_step=True)


def test_objective_step_not_with_the_records_nor_with_restart():
    with pytest.raises(AssertionError, match='objective_step cannot be combined with dual_function'):
        build(dual_function=True)
    with pytest.raises(AssertionError, match='objective_step cannot be combined with tree_record'):
        build(tree_record=True)
    with pytest.raises(AssertionError, match='restart needs a search run with frontier_batch and tree_record=True'):
        build().restart(None)
    with pytest.raises(AssertionError, match='restart overrides are'):   # (nor can a restart turn it on)
        bb = build(objective_step=None, tree_record=True)
        bb.status = 'optimal'
        bb.restart(None, objective_step=True)


def test_option_is_off_by_default():
    on = build()
    assert isinstance(on._objective_step, float) and on._objective_step > 0 and on.objective_step_stats is None
    assert build(objective_step=2)._objective_step == 2 and build(objective_step=0.25)._objective_step == 0.25
    plain = build(objective_step=None)
    assert plain._objective_step is None and plain.objective_step_stats is None
    # (what it works beside)
    assert build(primal_heuristic=True, local_search=True, propagate=True, reduced_cost=True, host_spill=1 << 24, dive=8,
                 anchor=False)._objective_step == on._objective_step


# ---- objective_step_of -------------------------------------------------------------------------------------------
def generator_model(c=None, ints=None):
    A, b, c0, l, u, ints0 = random_dense_milp_arrays(40, 20, seed=0)
    c = c0 if c is None else c
    return MILPInstance(A=A, b=b, c=c, l=l, u=u, sense=['Min', '>='], integerIndices=ints0 if ints is None else ints,
                        numVars=len(c)), c0


def test_objective_step_of():
    mdl, c = generator_model()
    assert objective_step_of(mdl) == 1.0
    for seed in range(4):   # (the generator's costs are 1 .. 10: their gcd is 1 on every instance in use)
        assert np.gcd.reduce(np.abs(random_dense_milp_arrays(40, 20, seed=seed)[2]).astype(np.int64)) == 1
    assert objective_step_of(generator_model(3 * c)[0]) == 3.0
    assert objective_step_of(generator_model(np.where(np.arange(40) % 2, 6.0, -4.0))[0]) == 2.0
    some = c * (np.arange(40) < 7)   # (columns without a cost do not count, continuous or not)
    assert objective_step_of(generator_model(12 * some, ints=list(range(7)))[0]) == 12.0 * np.gcd.reduce(np.abs(c[:7]).astype(np.int64))
    with pytest.raises(ValueError, match='column 39 has a cost and is not an integer column; pass the step'):
        objective_step_of(generator_model(ints=list(range(39)))[0])
    with pytest.raises(ValueError, match='the costs are not integers; pass the step'):
        objective_step_of(generator_model(c / 7)[0])
    with pytest.raises(ValueError, match='the objective is zero, it has no step; pass the step'):
        objective_step_of(generator_model(0 * c)[0])
    # a BranchAndBound as well as a model; True at construction is the same call
    bb = BranchAndBound(generator_model(3 * c)[0], PseudoCostBranchNode, pseudo_costs={}, frontier_batch=4, gomory_cuts=False,
                        objective_step=True)
    assert objective_step_of(bb) == 3.0 == bb._objective_step
    with pytest.raises(ValueError, match='pass the step'):
        BranchAndBound(generator_model(c / 7)[0], PseudoCostBranchNode, pseudo_costs={}, frontier_batch=4, gomory_cuts=False,
                       objective_step=True)
    given = BranchAndBound(generator_model(c / 2)[0], PseudoCostBranchNode, pseudo_costs={}, frontier_batch=4, gomory_cuts=False,
                           objective_step=0.5)
    assert given._objective_step == 0.5
    with pytest.raises(AssertionError, match='objective_step_of takes a BranchAndBound or a MILPInstance'):
        objective_step_of(c)
