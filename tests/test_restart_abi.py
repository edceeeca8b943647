"""Restarting a recorded search at another right-hand side, the parts that need no GPU: include/mipx_restart.h
against the ctypes table, the exported symbols, and what BranchAndBound.restart and the C entry refuse before
any device work."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from simple_mip_solver_amd import BranchAndBound, PseudoCostBranchNode, _ffi
from simple_mip_solver_amd.lp import CyLPArray
from tests.support.example_models import model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ['mipx_tree_create_restart', 'mipx_tree_restart_stats', 'mipx_tree_restart_seeds']


def restart_prototypes():
    text = open(os.path.join(ROOT, 'include', 'mipx_restart.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    text = re.sub(r'^\s*#.*$', '', text, flags=re.M)
    found = re.findall(r'([\w ]+?[\s*]+)(mipx_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;', text)
    return {name: (ret.strip(), [p.strip() for p in args.split(',') if p.strip() not in ('', 'void')])
            for ret, name, args in found}


def test_restart_header_and_signature_table_agree():
    scalars = {'int': C.c_int, 'int64_t': C.c_int64, 'size_t': C.c_size_t, 'double': C.c_double, 'void': None}

    def agrees(decl, ctype):
        if '*' in decl or '[' in decl:
            return ctype in (C.c_void_p, C.c_char_p) or (isinstance(ctype, type) and issubclass(ctype, C._Pointer))
        return ctype is scalars[decl.replace('const ', '').split()[0]]

    protos = restart_prototypes()
    assert sorted(protos) == sorted(_ffi.RESTART_SYMBOLS) == sorted(NAMES)
    for name, (ret, params) in protos.items():
        restype, argtypes = _ffi._RESTART_SIGNATURES[name]
        assert agrees(ret, restype), name
        assert len(params) == len(argtypes), name
        for k, (decl, ctype) in enumerate(zip(params, argtypes)):
            assert agrees(decl, ctype), f'{name} parameter {k} is `{decl}`, the table says {ctype}'


def test_new_symbols_overlap_no_existing_list():
    old = set(_ffi.SYMBOLS) | set(_ffi.SPILL_SYMBOLS) | set(_ffi.CUTMIG_SYMBOLS) | set(_ffi.DUALFN_SYMBOLS) | \
        set(_ffi.TREEREC_SYMBOLS) | set(_ffi.CGLP_SYMBOLS)
    assert not set(_ffi.RESTART_SYMBOLS) & old


def test_mipx_h_includes_the_restart_header_and_keeps_its_version():
    text = open(os.path.join(ROOT, 'include', 'mipx.h')).read()
    assert '#include "mipx_restart.h"' in text
    assert _ffi.lib().mipx_abi_version() == 1


def test_library_exports_the_restart_entries():
    L = _ffi.lib()
    for name in _ffi.RESTART_SYMBOLS:
        assert hasattr(L, name), name
        assert getattr(L, name).restype is _ffi._RESTART_SIGNATURES[name][0]


def test_stats_keys_cover_the_header_slots():
    text = open(os.path.join(ROOT, 'include', 'mipx_restart.h')).read()
    assert [int(k) for k in re.findall(r'\[(\d)\] ', text)] == list(range(8))
    assert len(_ffi.RESTART_STATS_KEYS) == 7   # ([7] is reserved)


def test_c_entries_refuse_null_arguments():
    L = _ffi.lib()
    out = C.c_void_p()
    assert L.mipx_tree_create_restart(None, None, C.byref(out)) == -1   # MIPX_EINVAL
    assert L.mipx_tree_restart_stats(None, None) == -1
    assert L.mipx_tree_restart_seeds(None, 0, None) == -1


def recorded(**extra):
    kw = dict(pseudo_costs={}, frontier_batch=4, gomory_cuts=False, tree_record=True)
    kw.update(extra)
    return BranchAndBound(model('small_branch'), PseudoCostBranchNode, **kw)


def rhs(bb, scale=1.0):
    return CyLPArray(scale * np.asarray(bb.model.b, dtype=np.float64))


def test_restart_needs_a_recorded_native_search():
    for kw in (dict(tree_record=None), dict(frontier_batch=None, tree_record=None)):
        bb = recorded(**kw)
        with pytest.raises(AssertionError, match='restart needs a search run with frontier_batch and tree_record=True'):
            bb.restart(rhs(bb))


def test_restart_needs_a_solved_source():
    bb = recorded()
    with pytest.raises(AssertionError, match='must solve this instance before using this method'):
        bb.restart(rhs(bb))


def solved_stub(**extra):
    """A source that counts as solved without a device: the refusals below come before any engine call."""
    bb = recorded(**extra)
    bb.status = 'stopped on iterations or time'
    return bb


def test_restart_not_with_comm():
    bb = solved_stub()
    with pytest.raises(AssertionError, match='restart cannot be combined with comm'):
        bb.restart(rhs(bb), comm=object())
    bb._comm = object()
    with pytest.raises(AssertionError, match='restart cannot be combined with comm'):
        bb.restart(rhs(bb))


def test_restart_rhs_type_and_shape():
    bb = solved_stub()
    with pytest.raises(AssertionError, match='this function only works with CyLP arrays'):
        bb.restart(np.asarray(bb.model.b))
    with pytest.raises(AssertionError, match='the shape of the RHS being added should match that of each node'):
        bb.restart(CyLPArray(np.zeros(len(bb.model.b) + 1)))


@pytest.mark.parametrize('value', [True, 1 << 20])
def test_restart_takes_no_dual_function(value):
    bb = solved_stub()
    with pytest.raises(AssertionError, match='dual_function is not available for a restarted search'):
        bb.restart(rhs(bb), dual_function=value)


def test_restart_overrides_are_a_closed_set():
    bb = solved_stub()
    with pytest.raises(AssertionError, match="restart overrides are .*not \\['pool_capacity'\\]"):
        bb.restart(rhs(bb), pool_capacity=1 << 10)
    with pytest.raises(AssertionError, match='at most the frontier_batch of its source'):
        bb.restart(rhs(bb), frontier_batch=8)


def test_default_has_no_restart_stats():
    assert recorded().restart_stats is None
