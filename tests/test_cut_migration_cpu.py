"""Node migration in cut-round mode, the parts that need no GPU: the exchange decision on records with
[13..15] set (include/mipx.h, mipx_exchange_decide), include/mipx_cutmig.h against its ctypes table, the
exported symbols, and the arguments BranchAndBound refuses."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from simple_mip_solver_amd import BranchAndBound, PseudoCostBranchNode, _ffi
from tests.support.example_models import model
from tests.test_parallel_cpu import record

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 6


def cut_record(open_nodes, kc, region=1000, cuts=1.0, **kw):
    r = record(N, open_nodes=open_nodes, **kw)
    r[13], r[14], r[15] = region, kc, cuts
    return r


def test_cut_mode_moves_when_every_rank_has_the_same_kc():
    recs = np.stack([cut_record(200, 64), cut_record(0, 64)])
    d = _ffi.exchange_decide(recs, N)
    assert d['moves'] == [(0, 1, 100)]
    # the same records without [13..15] decide exactly the same
    plain = recs.copy()
    plain[:, 13:16] = 0.0
    assert _ffi.exchange_decide(plain, N) == d


@pytest.mark.parametrize('kcs', [(64, 0), (0, 64), (0, 0), (64, 32), (32, 64)])
def test_cut_mode_moves_nothing_unless_every_kc_agrees(kcs):
    recs = np.stack([cut_record(200, kcs[0]), cut_record(0, kcs[1])])
    d = _ffi.exchange_decide(recs, N)
    assert d['moves'] == [] and d['reason'] == 0


def test_cut_mode_gate_with_three_ranks():
    recs = np.stack([cut_record(300, 16), cut_record(0, 16), cut_record(0, 16)])
    d = _ffi.exchange_decide(recs, N)
    assert len(d['moves']) == 2 and all(mv[0] == 0 for mv in d['moves'])
    assert sorted(mv[1] for mv in d['moves']) == [1, 2]    # at most one donation per receiver
    recs[2, 14] = 0.0                                       # one rank with cut migration off: nobody moves
    assert _ffi.exchange_decide(recs, N)['moves'] == []


def test_mixed_cut_flags_move_nothing():
    recs = np.stack([cut_record(200, 64), cut_record(0, 64, cuts=0.0)])
    assert _ffi.exchange_decide(recs, N)['moves'] == []


def test_zeroed_slots_decide_as_today():
    recs = np.stack([record(N, open_nodes=500, batch=8), record(N, open_nodes=2, batch=8, room=40),
                     record(N, open_nodes=0, batch=8)])
    d = _ffi.exchange_decide(recs, N)
    assert d['moves'] == [(0, 1, 40), (0, 2, 230)]
    assert _ffi.exchange_decide(recs, N, allow_migration=False)['moves'] == []


def test_cut_mode_still_honours_allow_migration_and_room():
    recs = np.stack([cut_record(200, 64), cut_record(0, 64, room=7)])
    assert _ffi.exchange_decide(recs, N)['moves'] == [(0, 1, 7)]
    assert _ffi.exchange_decide(recs, N, allow_migration=False)['moves'] == []


def cutmig_prototypes():
    text = open(os.path.join(ROOT, 'include', 'mipx_cutmig.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    found = re.findall(r'([\w ]+?[\s*]+)(mipx_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;', text)
    return {name: (ret.strip(), [p.strip() for p in args.split(',') if p.strip() not in ('', 'void')])
            for ret, name, args in found}


def test_cutmig_header_and_signature_table_agree():
    scalars = {'int': C.c_int, 'int64_t': C.c_int64, 'size_t': C.c_size_t, 'double': C.c_double, 'void': None}

    def agrees(decl, ctype):
        if '*' in decl or '[' in decl:
            return ctype in (C.c_void_p, C.c_char_p) or (isinstance(ctype, type) and issubclass(ctype, C._Pointer))
        return ctype is scalars[decl.replace('const ', '').split()[0]]

    protos = cutmig_prototypes()
    assert sorted(protos) == sorted(_ffi.CUTMIG_SYMBOLS)
    assert not set(protos) & (set(_ffi.SYMBOLS) | set(_ffi.SPILL_SYMBOLS))
    for name, (ret, params) in protos.items():
        restype, argtypes = _ffi._CUTMIG_SIGNATURES[name]
        assert agrees(ret, restype), name
        assert len(params) == len(argtypes), name
        for k, (decl, ctype) in enumerate(zip(params, argtypes)):
            assert agrees(decl, ctype), f'{name} parameter {k} is `{decl}`, the table says {ctype}'


def test_mipx_h_includes_the_cutmig_header():
    text = open(os.path.join(ROOT, 'include', 'mipx.h')).read()
    assert '#include "mipx_cutmig.h"' in text


def test_library_exports_the_cutmig_entries():
    L = _ffi.lib()
    for name in _ffi.CUTMIG_SYMBOLS:
        assert hasattr(L, name), name


def test_cut_migration_needs_comm():
    with pytest.raises(AssertionError, match='cut_migration needs comm'):
        BranchAndBound(model('small_branch'), PseudoCostBranchNode, pseudo_costs={}, frontier_batch=4,
                       cut_migration=True)


def test_cut_migration_needs_gomory_cuts():
    with pytest.raises(AssertionError, match='cut_migration needs gomory_cuts=True'):
        BranchAndBound(model('small_branch'), PseudoCostBranchNode, pseudo_costs={}, frontier_batch=4, comm=object(),
                       gomory_cuts=False, cut_migration=True)


@pytest.mark.parametrize('bad', [0, -1, 1.5, False, 'yes'])
def test_cut_migration_values(bad):
    with pytest.raises(AssertionError, match='cut_migration is None, True or a positive number of rows'):
        BranchAndBound(model('small_branch'), PseudoCostBranchNode, pseudo_costs={}, frontier_batch=4, comm=object(),
                       cut_migration=bad)
