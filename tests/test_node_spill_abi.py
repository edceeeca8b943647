"""Host spill of the frontier engine, the parts that need no GPU: include/mipx_spill.h against the ctypes
table, the exported symbols, and the arguments BranchAndBound refuses."""
import ctypes as C
import os
import re

import pytest

from simple_mip_solver_amd import BranchAndBound, PseudoCostBranchNode, _ffi
from tests.support.example_models import model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def spill_prototypes():
    text = open(os.path.join(ROOT, 'include', 'mipx_spill.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    found = re.findall(r'([\w ]+?[\s*]+)(mipx_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;', text)
    return {name: (ret.strip(), [p.strip() for p in args.split(',') if p.strip() not in ('', 'void')])
            for ret, name, args in found}


def test_spill_header_and_signature_table_agree():
    scalars = {'int': C.c_int, 'int64_t': C.c_int64, 'size_t': C.c_size_t, 'double': C.c_double, 'void': None}

    def agrees(decl, ctype):
        if '*' in decl or '[' in decl:
            return ctype in (C.c_void_p, C.c_char_p) or (isinstance(ctype, type) and issubclass(ctype, C._Pointer))
        return ctype is scalars[decl.replace('const ', '').split()[0]]

    protos = spill_prototypes()
    assert sorted(protos) == sorted(_ffi.SPILL_SYMBOLS)
    assert not set(protos) & set(_ffi.SYMBOLS)
    for name, (ret, params) in protos.items():
        restype, argtypes = _ffi._SPILL_SIGNATURES[name]
        assert agrees(ret, restype), name
        assert len(params) == len(argtypes), name
        for k, (decl, ctype) in enumerate(zip(params, argtypes)):
            assert agrees(decl, ctype), f'{name} parameter {k} is `{decl}`, the table says {ctype}'


def test_mipx_h_includes_the_spill_header():
    text = open(os.path.join(ROOT, 'include', 'mipx.h')).read()
    assert '#include "mipx_spill.h"' in text


def test_library_exports_the_spill_entries():
    L = _ffi.lib()
    for name in _ffi.SPILL_SYMBOLS:
        assert hasattr(L, name), name


def test_host_spill_needs_frontier_batch():
    with pytest.raises(AssertionError, match='host_spill needs frontier_batch'):
        BranchAndBound(model('small_branch'), PseudoCostBranchNode, pseudo_costs={}, host_spill=True)


def test_host_spill_not_with_comm():
    with pytest.raises(AssertionError, match='host_spill cannot be combined with comm'):
        BranchAndBound(model('small_branch'), PseudoCostBranchNode, pseudo_costs={}, frontier_batch=4, comm=object(),
                       host_spill=True)


@pytest.mark.parametrize('bad', [0, -1, 1.5, False, 'yes'])
def test_host_spill_values(bad):
    with pytest.raises(AssertionError, match='host_spill is None, True or a positive number of bytes'):
        BranchAndBound(model('small_branch'), PseudoCostBranchNode, pseudo_costs={}, frontier_batch=4, host_spill=bad)
