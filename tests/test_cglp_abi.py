"""Disjunctive separation, the parts that need no GPU: include/mipx_cglp.h against the ctypes table, the
exported symbols, and what the DisjunctiveSeparator constructor refuses."""
import ctypes as C
import os
import re

import pytest

from simple_mip_solver_amd import BranchAndBound, DisjunctiveSeparator, PseudoCostBranchNode, _ffi
from tests.support.example_models import model, std_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ['mipx_tree_support_open', 'mipx_tree_support_eval', 'mipx_tree_support_leaves', 'mipx_tree_support_stats',
         'mipx_tree_support_close']


def cglp_prototypes():
    text = open(os.path.join(ROOT, 'include', 'mipx_cglp.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    text = re.sub(r'^\s*#.*$', '', text, flags=re.M)
    found = re.findall(r'([\w ]+?[\s*]+)(mipx_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;', text)
    return {name: (ret.strip(), [p.strip() for p in args.split(',') if p.strip() not in ('', 'void')])
            for ret, name, args in found}


def test_cglp_header_and_signature_table_agree():
    scalars = {'int': C.c_int, 'int64_t': C.c_int64, 'size_t': C.c_size_t, 'double': C.c_double, 'void': None}

    def agrees(decl, ctype):
        if '*' in decl or '[' in decl:
            return ctype in (C.c_void_p, C.c_char_p) or (isinstance(ctype, type) and issubclass(ctype, C._Pointer))
        return ctype is scalars[decl.replace('const ', '').split()[0]]

    protos = cglp_prototypes()
    assert sorted(protos) == sorted(_ffi.CGLP_SYMBOLS) == sorted(NAMES)
    for name, (ret, params) in protos.items():
        restype, argtypes = _ffi._CGLP_SIGNATURES[name]
        assert agrees(ret, restype), name
        assert len(params) == len(argtypes), name
        for k, (decl, ctype) in enumerate(zip(params, argtypes)):
            assert agrees(decl, ctype), f'{name} parameter {k} is `{decl}`, the table says {ctype}'


def test_new_symbols_overlap_no_existing_list():
    old = set(_ffi.SYMBOLS) | set(_ffi.SPILL_SYMBOLS) | set(_ffi.CUTMIG_SYMBOLS) | set(_ffi.DUALFN_SYMBOLS) | \
        set(_ffi.TREEREC_SYMBOLS)
    assert not set(_ffi.CGLP_SYMBOLS) & old


def test_block_constants_match_the_kernels():
    text = open(os.path.join(ROOT, 'simple_mip_solver_amd', 'csrc', 'cglp_kernels.hip.h')).read()
    assert int(re.search(r'kSupHead = (\d+)', text).group(1)) == _ffi.CGLP_HEAD
    assert int(re.search(r'kSupMaxP = (\d+)', text).group(1)) == _ffi.CGLP_MAX_POINTS
    head = open(os.path.join(ROOT, 'include', 'mipx_cglp.h')).read()
    assert f'{_ffi.CGLP_HEAD} + max_points (n + 2) doubles' in head and f'max_points <= {_ffi.CGLP_MAX_POINTS}' in head


def test_mipx_h_includes_the_cglp_header():
    text = open(os.path.join(ROOT, 'include', 'mipx.h')).read()
    assert '#include "mipx_cglp.h"' in text


def test_library_exports_the_cglp_entries():
    L = _ffi.lib()
    for name in _ffi.CGLP_SYMBOLS:
        assert hasattr(L, name), name
        assert getattr(L, name).restype is _ffi._CGLP_SIGNATURES[name][0]


def recorded(factory=lambda: model('small_branch'), **kw):
    return BranchAndBound(factory(), PseudoCostBranchNode, pseudo_costs={}, frontier_batch=4, gomory_cuts=False,
                          tree_record=True, **kw)


def as_if_solved(bb):
    """What the constructor takes for a finished native search, without a GPU: the tree still is the root alone."""
    bb._native, bb._native_stats = object(), dict(status=0)
    return bb


def test_refuses_what_is_not_a_branch_and_bound():
    with pytest.raises(AssertionError, match='bb must be a BranchAndBound instance'):
        DisjunctiveSeparator(object(), 0)


def test_refuses_a_python_loop_search():
    bb = BranchAndBound(model('small_branch'), PseudoCostBranchNode, pseudo_costs={}, gomory_cuts=False)
    with pytest.raises(AssertionError, match='needs a native search: solve the BranchAndBound with frontier_batch'):
        DisjunctiveSeparator(bb, 0)


def test_refuses_a_search_without_tree_record():
    bb = BranchAndBound(model('small_branch'), PseudoCostBranchNode, pseudo_costs={}, frontier_batch=4, gomory_cuts=False)
    with pytest.raises(AssertionError, match='reads the recorded tree: pass tree_record=True'):
        DisjunctiveSeparator(bb, 0)


def test_refuses_an_unsolved_search():
    with pytest.raises(AssertionError, match='bb must be solved before a disjunction is read from its tree'):
        DisjunctiveSeparator(recorded(), 0)


def test_refuses_a_root_outside_the_tree():
    with pytest.raises(AssertionError, match='root node of the disjunction must be present in B & B tree'):
        DisjunctiveSeparator(as_if_solved(recorded()), 5)


def test_refuses_an_infinite_bound():
    bb = as_if_solved(recorded(lambda: std_model('small_branch')))
    with pytest.raises(AssertionError, match='every column of the subtree root must have finite bounds'):
        DisjunctiveSeparator(bb, 0)


@pytest.mark.parametrize('kw', [dict(depth=0), dict(depth=1.5), dict(tol=0.0), dict(max_rounds=0), dict(points_per_round=0),
                                dict(points_per_round=2000)])
def test_refuses_bad_parameters(kw):
    with pytest.raises(AssertionError):
        DisjunctiveSeparator(as_if_solved(recorded()), 0, **kw)
