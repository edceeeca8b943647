"""The C-ABI library loads and exports every symbol include/mipx.h declares (no compute calls:
this runs where there is no GPU), and fails loudly instead of falling back."""
import ctypes as C
import os
import re

import pytest

from simple_mip_solver_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, 'include', 'mipx.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b(mipx_[a-z0-9_]+)\s*\(', text)))


def test_header_and_binding_agree():
    assert declared_symbols() == sorted(_ffi.SYMBOLS)


def declared_prototypes():
    """{name: (return type, [parameter declarations])} of every function include/mipx.h declares."""
    text = open(os.path.join(ROOT, 'include', 'mipx.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    found = re.findall(r'([\w ]+?[\s*]+)(mipx_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;', text)
    return {name: (ret.strip(), [p.strip() for p in args.split(',') if p.strip() not in ('', 'void')])
            for ret, name, args in found}


def test_signature_table_matches_the_header():
    """Every _ffi._SIGNATURES entry has the header's arity, parameter types and return type (no library
    load: a wrong c_int against an int64_t / size_t or a missing restype shows here)."""
    scalars = {'int': C.c_int, 'int64_t': C.c_int64, 'size_t': C.c_size_t, 'double': C.c_double,
               'void': None, 'mipx_tree_hook': _ffi.TREE_HOOK}

    def agrees(decl, ctype):
        if '*' in decl or '[' in decl:   # any pointer, array parameter or opaque handle
            return ctype in (C.c_void_p, C.c_char_p) or (isinstance(ctype, type) and issubclass(ctype, C._Pointer))
        return ctype is scalars[decl.replace('const ', '').split()[0]]

    protos = declared_prototypes()
    assert len(protos) == len(_ffi._SIGNATURES) == 70
    for name, (ret, params) in protos.items():
        restype, argtypes = _ffi._SIGNATURES[name]
        assert agrees(ret, restype), f'{name} returns {ret}, the table says {restype}'
        assert len(params) == len(argtypes), f'{name}: {len(params)} parameters, the table has {len(argtypes)}'
        for k, (decl, ctype) in enumerate(zip(params, argtypes)):
            assert agrees(decl, ctype), f'{name} parameter {k} is `{decl}`, the table says {ctype}'


def test_library_exports_every_declared_symbol():
    L = _ffi.lib()
    for name in declared_symbols():
        assert hasattr(L, name), f'libmipx.so does not export {name}'
    assert L.mipx_abi_version() == 1


def test_kernel_dispatch_table():
    assert _ffi.kernel_name(32, 64) == 'lp_dual_simplex<1,8,4>'
    assert _ffi.kernel_name(128, 256) == 'lp_dual_simplex<7,5,16>'
    assert _ffi.kernel_name(129, 256) == 'lp_dual_simplex<7,7,16>'
    assert _ffi.kernel_name(512, 1024) == 'lp_dual_simplex_big'   # streamed from HBM
    with pytest.raises(_ffi.MipxError, match='MIPX_ETOOBIG'):
        _ffi.kernel_name(512, 2048)


def test_no_silent_cpu_fallback():
    """Without a GPU the product path raises; with one it creates a context."""
    L = _ffi.lib()
    if L.mipx_device_count() == 0:
        with pytest.raises(_ffi.MipxError, match='no CPU fallback'):
            _ffi.Context(0)
        from simple_mip_solver_amd import lp
        from tests.support.example_models import model
        lp.set_backend(None)
        with pytest.raises(_ffi.MipxError):
            model('small_branch').lp.dual()
    else:
        _ffi.Context(0).close()


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, 'simple_mip_solver_amd')
    for d, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(('.py', '.hip', '.h', '.cpp')):
                text = open(os.path.join(d, f)).read()
                assert 'import oracle' not in text and 'from oracle' not in text, f
                assert 'libmipx_oracle' not in text and 'mipx_oracle_' not in text, f
