"""A header of include/ against a ctypes signature table: the prototypes the header declares, and whether a C
declaration agrees with a ctypes type; and what make rebuilds the library for.  Test infrastructure only."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def prototypes(header):
    text = open(os.path.join(ROOT, 'include', header)).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    text = re.sub(r'^\s*#.*$', '', text, flags=re.M)
    found = re.findall(r'([\w ]+?[\s*]+)(mipx_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;', text)
    return {name: (ret.strip(), [p.strip() for p in args.split(',') if p.strip() not in ('', 'void')])
            for ret, name, args in found}


def agrees(decl, ctype):
    scalars = {'int': C.c_int, 'int64_t': C.c_int64, 'size_t': C.c_size_t, 'double': C.c_double, 'void': None}
    if '*' in decl or '[' in decl:
        return ctype in (C.c_void_p, C.c_char_p) or (isinstance(ctype, type) and issubclass(ctype, C._Pointer))
    return ctype is scalars[decl.replace('const ', '').split()[0]]


def library_prerequisites():
    """The files csrc/Makefile rebuilds libmipx.so for, as make expands them (the public headers are taken by pattern)."""
    csrc = os.path.join(ROOT, 'simple_mip_solver_amd', 'csrc')
    db = subprocess.run(['make', '-C', csrc, '-pnq', 'libmipx.so'], capture_output=True, text=True).stdout
    return {os.path.normpath(os.path.join(csrc, f)) for f in re.search(r'^libmipx\.so:(.*)$', db, flags=re.M).group(1).split()}
