"""Reader of ``include/wc_kernels.h``: the header is the one declaration of the C ABI, and the ctypes
binding (``_native``) is read from its text -- the ``WC_*`` constants, every struct as a
``ctypes.Structure`` and every prototype as (restype, argtypes).

Not a C parser: it takes exactly the subset the header uses and raises ``AbiError`` with the offending
text on anything else (an unknown type, a function pointer, a union, a bit-field, a declaration it
cannot split).  A pure function of the text; ``_native`` runs it once per process.
"""
import ctypes
import re
from typing import Dict, List, NamedTuple, Tuple

_SCALARS = {'int': ctypes.c_int, 'float': ctypes.c_float, 'double': ctypes.c_double, 'int64_t': ctypes.c_int64,
            'uint64_t': ctypes.c_uint64}
_POINTEES = set(_SCALARS) | {'void', 'char', 'unsigned long long'}  # what a plain (c_void_p) pointer may point at
_RETURNS = {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'const char*': ctypes.c_char_p}

_DEFINE = re.compile(r'#define\s+(\w+)\s*(.*)')
_INT = re.compile(r'\((-?\d+)\)|(-?\d+)')
_STRUCT = re.compile(r'typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*')
_PROTO = re.compile(r'(.+?)\s*\b(\w+)\s*\(([^()]*)\)\s*')
_DECL = re.compile(r'(const\s+)?(.+?)\s*(\*?)\s*((?:\w+(?:\[\w+\])?\s*,\s*)*\w+(?:\[\w+\])?)')


class AbiError(ValueError):
    pass


class Abi(NamedTuple):
    constants: Dict[str, int]
    structs: Dict[str, type]  # C name -> ctypes.Structure subclass, in header order
    functions: Dict[str, Tuple[object, List[object]]]  # name -> (restype, argtypes), in header order


def _preprocess(text: str, constants: Dict[str, int]) -> str:
    """The declarations alone: comments and the preprocessor lines removed, the #defines collected."""
    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)
    out, guard = [], None
    for line in text.splitlines():
        s = line.strip()
        if not s.startswith('#'):
            if s not in ('extern "C" {', '}'):  # the extern "C" block's own two lines
                out.append(line)
            continue
        m = _DEFINE.fullmatch(s)
        if m and m.group(1) == guard and not m.group(2):
            continue
        if m:
            v = _INT.fullmatch(m.group(2).strip())
            if not (m.group(1).startswith('WC_') and v):
                raise AbiError(f'not a WC_<NAME> <integer> constant: {s!r}')
            constants[m.group(1)] = int(v.group(1) or v.group(2))
        elif s.startswith('#ifndef '):
            guard = s.split()[1]
        elif not re.fullmatch(r'#include\s*<stdint\.h>|#ifdef\s+__cplusplus|#endif', s):
            raise AbiError(f'unknown preprocessor line: {s!r}')
    return '\n'.join(out)


def _split(decl: str, what: str):
    """(type name, '*' or '', [declarators]) of one field or parameter declaration (const dropped)."""
    for bad, why in (('(', 'function pointer'), (':', 'bit-field')):
        if bad in decl:
            raise AbiError(f'{why} in {what}: {decl!r}')
    m = _DECL.fullmatch(decl)
    if not m:
        raise AbiError(f'cannot split {what}: {decl!r}')
    names = [d.strip() for d in m.group(4).split(',')]
    if m.group(3) and len(names) > 1:
        raise AbiError(f'several declarators of a pointer type in {what}: {decl!r}')
    return ' '.join(m.group(2).split()), m.group(3), names


def _ctype(ty: str, star: str, structs: Dict[str, type], decl: str, struct_pointers: bool):
    if ty not in structs and ty not in (_POINTEES if star else _SCALARS):
        raise AbiError(f'unknown type {ty!r} in {decl!r}')
    if not star:
        return structs[ty] if ty in structs else _SCALARS[ty]
    return ctypes.POINTER(structs[ty]) if struct_pointers and ty in structs else ctypes.c_void_p


def _struct(name: str, body: str, constants: Dict[str, int], structs: Dict[str, type]) -> type:
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(';'))):
        ty, star, names = _split(decl, f'struct {name}')
        ct = _ctype(ty, star, structs, decl, struct_pointers=False)  # every pointer field is c_void_p
        for d in names:
            fname, _, bound = d.rstrip(']').partition('[')
            if bound and not (bound.isdigit() or bound in constants):
                raise AbiError(f'array bound {bound!r} is not an integer constant: {decl!r}')
            fields.append((fname, ct * int(constants.get(bound, bound)) if bound else ct))
    return type(name, (ctypes.Structure, ), {'_fields_': fields})


def _function(ret: str, params: str, structs: Dict[str, type], decl: str):
    ret = re.sub(r'\s*\*', '*', ' '.join(ret.split()))
    if ret not in _RETURNS:
        raise AbiError(f'unknown return type {ret!r}: {decl!r}')
    argtypes = []
    for p in ([] if params.strip() == 'void' else params.split(',')):
        ty, star, names = _split(p.strip(), 'prototype')
        if len(names) > 1 or '[' in names[0] or ty in structs and not star:
            raise AbiError(f'cannot split parameter {p.strip()!r}: {decl!r}')
        argtypes.append(_ctype(ty, star, structs, decl, struct_pointers=True))
    return _RETURNS[ret], argtypes


def read(text: str) -> Abi:
    """The constants, structs and functions the header text declares (AbiError on anything else)."""
    abi = Abi({}, {}, {})
    rest = _preprocess(text, abi.constants)
    bad = re.search(r'\b(union|enum)\b[^;]*', rest)
    if bad:
        raise AbiError(f'{bad.group(1)} is not supported: {bad.group(0)!r}')
    for decl in filter(None, (d.strip() for d in re.split(r';(?![^{]*\})', rest))):  # ';' outside braces
        m = _STRUCT.fullmatch(decl)
        if m:
            if m.group(1) != m.group(3) or m.group(1) in abi.structs:
                raise AbiError(f'struct tag and typedef differ, or declared twice: {decl!r}')
            abi.structs[m.group(1)] = _struct(m.group(1), m.group(2), abi.constants, abi.structs)
            continue
        m = _PROTO.fullmatch(decl)
        if not m:
            why = 'function pointer in' if decl.count('(') > 1 and '{' not in decl else 'cannot split'
            raise AbiError(f'{why} declaration: {decl!r}')
        if m.group(2) in abi.functions:
            raise AbiError(f'declared twice: {decl!r}')
        abi.functions[m.group(2)] = _function(m.group(1), m.group(3), abi.structs, decl)
    return abi
