"""Reader of include/rvt_hip.h: the header is the single source of the ctypes binding (prototypes, structs, the rows of the device
tables, the records the device writes back and the enumerators).

A plain regex reader of that header's dialect, not a C parser, and loud: a type it does not know, or text left over after the
typedef'd structs, the enums and the prototypes are taken out, raises.  The header is read once, when this module is imported."""
from __future__ import annotations

import ctypes
import os
import re
from typing import Dict, List, NamedTuple, Optional, Tuple

HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'rvt_hip.h')

_SCALARS = {'int': ctypes.c_int, 'unsigned': ctypes.c_uint, 'float': ctypes.c_float, 'double': ctypes.c_double,
            'size_t': ctypes.c_size_t, 'long long': ctypes.c_longlong}
_POINTEES = set(_SCALARS) | {'void', 'char', 'unsigned char', 'signed char'}       # what a `T*` may point to besides a struct
_STRUCT = re.compile(r'typedef\s+struct\s*(\w*)\s*\{([^{}]*)\}\s*(\w+)\s*;')     # no tag: a record the device writes (RECORDS)
_ENUM = re.compile(r'\benum\s*\{([^{}]*)\}\s*;')
_ENUMERATOR = re.compile(r'([A-Za-z_]\w*)(?:\s*=\s*(-?\d+))?')
_ARRAY = re.compile(r'\[\s*(\d+)\s*\]\s*\Z')
_SCAFFOLD = re.compile(r'extern\s+"C"\s*\{|\}\s*\Z')
_PROTO = re.compile(r'([^()]+)\(([^()]*)\)')


class Proto(NamedTuple):
    restype: Optional[type]
    argtypes: List[type]
    argnames: Tuple[str, ...]


def _decl(text: str) -> Tuple[str, int, str, Optional[int]]:
    """`const float *w` (const already gone) -> ('float', 1, 'w', None); `int d[5]` -> ('int', 0, 'd', 5)."""
    m = _ARRAY.search(text)
    head, _, name = ' '.join((text[:m.start()] if m else text).replace('*', ' * ').split()).rpartition(' ')
    base = ' '.join(head.replace('*', ' ').split())
    if not base or not name.isidentifier():
        raise RuntimeError(f'rvt_hip.h reader: cannot read the declarator {text.strip()!r}')
    return base, head.count('*'), name, int(m.group(1)) if m else None


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


def _enums(text: str) -> Dict[str, int]:
    """Enumerators of every `enum { A = 0, B, ... };` of a comment-free text: explicit decimal values and auto-increment."""
    out: Dict[str, int] = {}
    for body in _ENUM.findall(text):
        nxt = 0
        for item in filter(None, map(str.strip, body.split(','))):
            m = _ENUMERATOR.fullmatch(item)
            if m is None or m.group(1) in out:
                raise RuntimeError(f'rvt_hip.h reader: cannot read the enumerator {item!r}')
            out[m.group(1)] = nxt = int(m.group(2)) if m.group(2) else nxt
            nxt += 1
    return out


def parse(text: str) -> Tuple[Dict[str, type], Dict[str, Proto], Dict[str, int]]:
    """(structs by name, prototypes by name, enumerators by name) of a header text, each in declaration order."""
    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)
    text = re.sub(r'^[ \t]*#.*$', ' ', text, flags=re.M)
    text = re.sub(r'\bconst\b', ' ', text)
    structs: Dict[str, type] = {}
    for name, body, alias in _STRUCT.findall(text):
        if name and name != alias:
            raise RuntimeError(f'rvt_hip.h reader: struct {name} is typedef\'d as {alias}')
        tagged, name = bool(name), alias
        fields = []
        for stmt in filter(str.strip, body.split(';')):
            first, *more = stmt.split(',')               # `int a, b` / `const float *w, *b`: one field per name
            base = _decl(first)[0]
            for piece in [first] + [f'{base} {p}' for p in more]:
                _, stars, field, count = _decl(piece)
                ty = _ctype(base, stars, structs, f'struct {name}', in_struct=True)
                fields.append((field, ty if count is None else ty * count))
        structs[name] = type(name, (ctypes.Structure,), {'_fields_': fields, '_tagged_': tagged,
                                                         '__doc__': f'`struct {name}` of include/rvt_hip.h'})
    enums = _enums(text)
    text = _SCAFFOLD.sub(' ', _ENUM.sub(' ', _STRUCT.sub(' ', text)))
    protos: Dict[str, Proto] = {}
    for stmt in filter(str.strip, text.split(';')):
        m = _PROTO.fullmatch(stmt.strip())
        if m is None:
            raise RuntimeError(f'rvt_hip.h reader: unrecognised declaration {stmt.strip()!r}')
        base, stars, name, count = _decl(m.group(1))
        params = m.group(2).strip()
        args = [_decl(p) for p in params.split(',')] if params not in ('', 'void') else []
        if count is not None or any(a[3] is not None for a in args):
            raise RuntimeError(f'rvt_hip.h reader: array in the prototype of {name} (arrays are struct fields only)')
        protos[name] = Proto(_ctype(base, stars, structs, name, is_return=True),
                             [_ctype(b, s, structs, name) for b, s, _, _ in args], tuple(a[2] for a in args))
    return structs, protos, enums


def fields(struct: type) -> Tuple[str, ...]:
    """Field names of a generated struct, in header order."""
    return tuple(f for f, _ in struct._fields_)


class LaunchArgs:
    """The positional arguments of one recorded launch under the header's parameter names: `a.M`, `a.T_steps`, `a.has('gates')`."""

    def __init__(self, name: str, args):
        proto = PROTOS[name]
        if len(proto.argnames) != len(args):
            raise TypeError(f'{name} takes {len(proto.argnames)} arguments ({", ".join(proto.argnames)}), the record has {len(args)}')
        self._name, self._args = name, dict(zip(proto.argnames, args))
        self._pointers = {n for n, ty in zip(proto.argnames, proto.argtypes) if ty is ctypes.c_void_p}

    def __getattr__(self, arg: str):             # (only reached for names that are not attributes of the object itself)
        try:
            return self._args[arg]
        except KeyError:
            raise AttributeError(f'{self._name} has no parameter {arg!r}') from None

    def has(self, pointer: str) -> bool:
        """Is this pointer argument present (not NULL)?"""
        if pointer not in self._pointers:
            raise TypeError(f'{pointer!r} is not a pointer parameter of {self._name}')
        return self._args[pointer] is not None


def _read() -> Tuple[Dict[str, type], Dict[str, Proto], Dict[str, int]]:
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


_ALL_STRUCTS, PROTOS, ENUMS = _read()
# what a host FILLS (host-side records, rows of the device tables: `typedef struct X {...} X;`) and what the device writes and a host
# only reads back (`typedef struct {...} X;`, no tag): the header's two directions
STRUCTS = {n: s for n, s in _ALL_STRUCTS.items() if s._tagged_}
RECORDS = {n: s for n, s in _ALL_STRUCTS.items() if not s._tagged_}
SIGS = {name: p.argtypes for name, p in PROTOS.items()}      # name -> ctypes types of the arguments, every prototype
