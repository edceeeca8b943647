"""The dual function of the frontier engine, the parts that need no GPU: include/mipx_dualfn.h against the
ctypes table, the exported symbols, and the arguments BranchAndBound refuses."""
import ctypes as C
import os
import re

import pytest

from simple_mip_solver_amd import BranchAndBound, PseudoCostBranchNode, _ffi
from tests.support.example_models import model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dualfn_prototypes():
    text = open(os.path.join(ROOT, 'include', 'mipx_dualfn.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    found = re.findall(r'([\w ]+?[\s*]+)(mipx_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;', text)
    return {name: (ret.strip(), [p.strip() for p in args.split(',') if p.strip() not in ('', 'void')])
            for ret, name, args in found}


def test_dualfn_header_and_signature_table_agree():
    scalars = {'int': C.c_int, 'int64_t': C.c_int64, 'size_t': C.c_size_t, 'double': C.c_double, 'void': None}

    def agrees(decl, ctype):
        if '*' in decl or '[' in decl:
            return ctype in (C.c_void_p, C.c_char_p) or (isinstance(ctype, type) and issubclass(ctype, C._Pointer))
        return ctype is scalars[decl.replace('const ', '').split()[0]]

    protos = dualfn_prototypes()
    assert sorted(protos) == sorted(_ffi.DUALFN_SYMBOLS) == sorted(
        ['mipx_tree_set_dual_record', 'mipx_tree_dual_function', 'mipx_tree_dual_function_stats',
         'mipx_tree_dual_records'])
    assert not set(protos) & (set(_ffi.SYMBOLS) | set(_ffi.SPILL_SYMBOLS) | set(_ffi.CUTMIG_SYMBOLS))
    for name, (ret, params) in protos.items():
        restype, argtypes = _ffi._DUALFN_SIGNATURES[name]
        assert agrees(ret, restype), name
        assert len(params) == len(argtypes), name
        for k, (decl, ctype) in enumerate(zip(params, argtypes)):
            assert agrees(decl, ctype), f'{name} parameter {k} is `{decl}`, the table says {ctype}'


def test_mipx_h_includes_the_dualfn_header():
    text = open(os.path.join(ROOT, 'include', 'mipx.h')).read()
    assert '#include "mipx_dualfn.h"' in text


def test_library_exports_the_dualfn_entries():
    L = _ffi.lib()
    for name in _ffi.DUALFN_SYMBOLS:
        assert hasattr(L, name), name
        assert getattr(L, name).restype is _ffi._DUALFN_SIGNATURES[name][0]


def test_dual_function_needs_frontier_batch():
    with pytest.raises(AssertionError, match='dual_function needs frontier_batch'):
        BranchAndBound(model('small_branch'), PseudoCostBranchNode, pseudo_costs={}, gomory_cuts=False,
                       dual_function=True)


def test_dual_function_not_with_comm():
    with pytest.raises(AssertionError, match='dual_function cannot be combined with comm'):
        BranchAndBound(model('small_branch'), PseudoCostBranchNode, pseudo_costs={}, frontier_batch=4, comm=object(),
                       gomory_cuts=False, dual_function=True)


def test_dual_function_not_with_cut_rounds():
    with pytest.raises(AssertionError, match='dual_function needs gomory_cuts=False'):
        BranchAndBound(model('small_branch'), PseudoCostBranchNode, pseudo_costs={}, frontier_batch=4,
                       dual_function=True)
    with pytest.raises(AssertionError, match='dual_function needs gomory_cuts=False'):
        BranchAndBound(model('small_branch'), PseudoCostBranchNode, pseudo_costs={}, frontier_batch=4,
                       gomory_cuts=True, dual_function=True)


@pytest.mark.parametrize('bad', [0, -1, 1.5, False, 'yes'])
def test_dual_function_values(bad):
    with pytest.raises(AssertionError, match='dual_function is None, True or a positive number of bytes'):
        BranchAndBound(model('small_branch'), PseudoCostBranchNode, pseudo_costs={}, frontier_batch=4,
                       gomory_cuts=False, dual_function=bad)


def test_dual_function_allows_spill_anchor_dive():
    bb = BranchAndBound(model('small_branch'), PseudoCostBranchNode, pseudo_costs={}, frontier_batch=4,
                        gomory_cuts=False, dual_function=1 << 20, host_spill=1 << 20, anchor=True, dive=2)
    assert bb.dual_function_stats is None


def test_without_dual_function_the_refusal_stays():
    from simple_mip_solver_amd import CyLPArray
    bb = BranchAndBound(model('small_branch'), PseudoCostBranchNode, pseudo_costs={}, frontier_batch=4,
                        gomory_cuts=False)
    bb.status = 'stopped on iterations or time'   # (as after a solve; no GPU needed for the refusal)
    with pytest.raises(AssertionError, match='the native frontier engine keeps no per-node duals; solve with '
                                             'frontier_batch=None'):
        bb.find_parameterized_dual_bound(CyLPArray([2.5, 4.5]))
