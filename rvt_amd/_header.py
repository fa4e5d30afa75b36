"""Reader of include/rvt_hip.h: the header is the single source of the ctypes binding (prototypes and structs).

A plain regex reader of that header's dialect, not a C parser, and loud: a type it does not know, or text left over after the
typedef'd structs and the prototypes are taken out, raises.  The header is read once, when this module is imported."""
from __future__ import annotations

import ctypes
import os
import re
from typing import Dict, List, NamedTuple, Optional, Tuple

HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'rvt_hip.h')

_SCALARS = {'int': ctypes.c_int, 'float': ctypes.c_float, 'double': ctypes.c_double, 'size_t': ctypes.c_size_t,
            'long long': ctypes.c_longlong}
_POINTEES = set(_SCALARS) | {'void', 'char', 'unsigned', 'unsigned char', 'signed char'}       # what a `T*` may point to besides a struct
_STRUCT = re.compile(r'typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;')
_SCAFFOLD = re.compile(r'extern\s+"C"\s*\{|enum\s*\{[^{}]*\}\s*;|\}\s*\Z')
_PROTO = re.compile(r'([^()]+)\(([^()]*)\)')


class Proto(NamedTuple):
    restype: Optional[type]
    argtypes: List[type]
    argnames: Tuple[str, ...]


def _decl(text: str) -> Tuple[str, int, str]:
    """`const float *w` (const already gone) -> ('float', 1, 'w')."""
    head, _, name = ' '.join(text.replace('*', ' * ').split()).rpartition(' ')
    base = ' '.join(head.replace('*', ' ').split())
    if not base or not name.isidentifier():
        raise RuntimeError(f'rvt_hip.h reader: cannot read the declarator {text.strip()!r}')
    return base, head.count('*'), name


def _ctype(base: str, stars: int, structs: Dict[str, type], where: str, in_struct: bool = False, is_return: bool = False):
    if base not in _POINTEES and base not in structs:
        raise RuntimeError(f'rvt_hip.h reader: unknown type {base!r} in {where}')
    if stars:
        if is_return and base == 'char' and stars == 1:
            return ctypes.c_char_p
        return ctypes.POINTER(structs[base]) if in_struct and stars == 1 and base in structs else ctypes.c_void_p
    if base in _SCALARS:
        return _SCALARS[base]
    if base in structs and in_struct:
        return structs[base]
    if base == 'void' and is_return:
        return None
    raise RuntimeError(f'rvt_hip.h reader: type {base!r} cannot be passed by value in {where}')


def parse(text: str) -> Tuple[Dict[str, type], Dict[str, Proto]]:
    """(structs by name, prototypes by name) of a header text, both in declaration order."""
    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)
    text = re.sub(r'^[ \t]*#.*$', ' ', text, flags=re.M)
    text = re.sub(r'\bconst\b', ' ', text)
    structs: Dict[str, type] = {}
    for name, body, alias in _STRUCT.findall(text):
        if name != alias:
            raise RuntimeError(f'rvt_hip.h reader: struct {name} is typedef\'d as {alias}')
        fields = []
        for stmt in filter(str.strip, body.split(';')):
            first, *more = stmt.split(',')               # `int a, b` / `const float *w, *b`: one field per name
            base = _decl(first)[0]
            for piece in [first] + [f'{base} {p}' for p in more]:
                _, stars, field = _decl(piece)
                fields.append((field, _ctype(base, stars, structs, f'struct {name}', in_struct=True)))
        structs[name] = type(name, (ctypes.Structure,), {'_fields_': fields, '__doc__': f'`struct {name}` of include/rvt_hip.h'})
    text = _SCAFFOLD.sub(' ', _STRUCT.sub(' ', text))
    protos: Dict[str, Proto] = {}
    for stmt in filter(str.strip, text.split(';')):
        m = _PROTO.fullmatch(stmt.strip())
        if m is None:
            raise RuntimeError(f'rvt_hip.h reader: unrecognised declaration {stmt.strip()!r}')
        base, stars, name = _decl(m.group(1))
        params = m.group(2).strip()
        args = [_decl(p) for p in params.split(',')] if params not in ('', 'void') else []
        protos[name] = Proto(_ctype(base, stars, structs, name, is_return=True),
                             [_ctype(b, s, structs, name) for b, s, _ in args], tuple(n for _, _, n in args))
    return structs, protos


def fields(struct: type) -> Tuple[str, ...]:
    """Field names of a generated struct, in header order."""
    return tuple(f for f, _ in struct._fields_)


def _read() -> Tuple[Dict[str, type], Dict[str, Proto]]:
    try:
        with open(HEADER_PATH) as f:
            return parse(f.read())
    except OSError as e:
        raise RuntimeError(f'{HEADER_PATH} cannot be read ({e}): rvt_amd derives its ctypes binding from that header') from None


def bind(lib: ctypes.CDLL) -> ctypes.CDLL:
    """Install the header's types on every entry point of a loaded library."""
    for name, p in PROTOS.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is missing -> loud
        fn.restype, fn.argtypes = p.restype, p.argtypes
    return lib


STRUCTS, PROTOS = _read()
SIGS = {name: p.argtypes for name, p in PROTOS.items()}      # name -> ctypes types of the arguments, every prototype
