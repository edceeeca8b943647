"""A header of include/ against a ctypes signature table: the prototypes the header declares, and whether a C
declaration agrees with a ctypes type.  Test infrastructure only."""
import ctypes as C
import os
import re

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
