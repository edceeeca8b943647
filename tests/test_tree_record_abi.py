"""The tree record of the frontier engine, the parts that need no GPU: include/mipx_treerec.h against the
ctypes table, the exported symbols, and the arguments BranchAndBound refuses."""
import ctypes as C
import os
import re

import pytest

from simple_mip_solver_amd import BranchAndBound, PseudoCostBranchNode, _ffi
from tests.support.example_models import model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ['mipx_tree_set_tree_record', 'mipx_tree_records', 'mipx_tree_node_bounds', 'mipx_tree_node_solve',
         'mipx_tree_record_stats']


def treerec_prototypes():
    text = open(os.path.join(ROOT, 'include', 'mipx_treerec.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    text = re.sub(r'^\s*#.*$', '', text, flags=re.M)
    found = re.findall(r'([\w ]+?[\s*]+)(mipx_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;', text)
    return {name: (ret.strip(), [p.strip() for p in args.split(',') if p.strip() not in ('', 'void')])
            for ret, name, args in found}


def test_treerec_header_and_signature_table_agree():
    scalars = {'int': C.c_int, 'int64_t': C.c_int64, 'size_t': C.c_size_t, 'double': C.c_double, 'void': None}

    def agrees(decl, ctype):
        if '*' in decl or '[' in decl:
            return ctype in (C.c_void_p, C.c_char_p) or (isinstance(ctype, type) and issubclass(ctype, C._Pointer))
        return ctype is scalars[decl.replace('const ', '').split()[0]]

    protos = treerec_prototypes()
    assert sorted(protos) == sorted(_ffi.TREEREC_SYMBOLS) == sorted(NAMES)
    for name, (ret, params) in protos.items():
        restype, argtypes = _ffi._TREEREC_SIGNATURES[name]
        assert agrees(ret, restype), name
        assert len(params) == len(argtypes), name
        for k, (decl, ctype) in enumerate(zip(params, argtypes)):
            assert agrees(decl, ctype), f'{name} parameter {k} is `{decl}`, the table says {ctype}'


def test_new_symbols_overlap_no_existing_list():
    old = set(_ffi.SYMBOLS) | set(_ffi.SPILL_SYMBOLS) | set(_ffi.CUTMIG_SYMBOLS) | set(_ffi.DUALFN_SYMBOLS)
    assert not set(_ffi.TREEREC_SYMBOLS) & old


def test_record_flags_match_the_header():
    text = open(os.path.join(ROOT, 'include', 'mipx_treerec.h')).read()
    flags = {name: int(value) for name, value in re.findall(r'#define MIPX_(TR_[A-Z_]+) (\d+)', text)}
    assert flags == {'TR_MIP_FEASIBLE': _ffi.TR_MIP_FEASIBLE, 'TR_HAS_CHILDREN': _ffi.TR_HAS_CHILDREN,
                     'TR_CLOSED_AT_POP': _ffi.TR_CLOSED_AT_POP, 'TR_OPEN': _ffi.TR_OPEN, 'TR_PROBED': _ffi.TR_PROBED}


def test_mipx_h_includes_the_treerec_header():
    text = open(os.path.join(ROOT, 'include', 'mipx.h')).read()
    assert '#include "mipx_treerec.h"' in text


def test_library_exports_the_treerec_entries():
    L = _ffi.lib()
    for name in _ffi.TREEREC_SYMBOLS:
        assert hasattr(L, name), name
        assert getattr(L, name).restype is _ffi._TREEREC_SIGNATURES[name][0]


def test_tree_record_needs_frontier_batch():
    with pytest.raises(AssertionError, match='tree_record needs frontier_batch'):
        BranchAndBound(model('small_branch'), PseudoCostBranchNode, pseudo_costs={}, gomory_cuts=False,
                       tree_record=True)


def test_tree_record_not_with_comm():
    with pytest.raises(AssertionError, match='tree_record cannot be combined with comm'):
        BranchAndBound(model('small_branch'), PseudoCostBranchNode, pseudo_costs={}, frontier_batch=4, comm=object(),
                       gomory_cuts=False, tree_record=True)


def test_tree_record_not_with_cut_rounds():
    for kwargs in ({}, dict(gomory_cuts=True)):
        with pytest.raises(AssertionError, match='tree_record needs gomory_cuts=False: recorded nodes carry no cut rows'):
            BranchAndBound(model('small_branch'), PseudoCostBranchNode, pseudo_costs={}, frontier_batch=4,
                           tree_record=True, **kwargs)


@pytest.mark.parametrize('bad', [0, 1, False, 'yes', 1 << 20])
def test_tree_record_values(bad):
    with pytest.raises(AssertionError, match='tree_record is None or True'):
        BranchAndBound(model('small_branch'), PseudoCostBranchNode, pseudo_costs={}, frontier_batch=4,
                       gomory_cuts=False, tree_record=bad)


def test_tree_record_allows_dual_function_spill_anchor_dive():
    bb = BranchAndBound(model('small_branch'), PseudoCostBranchNode, pseudo_costs={}, frontier_batch=4,
                        gomory_cuts=False, tree_record=True, dual_function=1 << 20, host_spill=1 << 20, anchor=True,
                        dive=2)
    assert bb.tree_record_stats is None
    assert list(bb.tree.nodes) == [0]   # (until a solve: the root alone, as without the option)


def test_default_is_off():
    bb = BranchAndBound(model('small_branch'), PseudoCostBranchNode, pseudo_costs={}, frontier_batch=4,
                        gomory_cuts=False)
    assert bb._tree_record is None and bb.tree_record_stats is None
