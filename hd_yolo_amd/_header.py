"""Reader of include/hdyolo.h: the header is the one description of the C ABI, and the ctypes binding (_lib.py) is derived from it.

`parse(text)` gives a Header with
    functions  {name: (restype, [argtypes])}            ctypes types, as `lib.<name>.restype / .argtypes` take them
    params     {name: [(parameter name, const)]}        beside `functions[name][1]`, position by position
    structs    {typedef name: ctypes.Structure class}   the header's field names and order
    constants  {HDY_NAME: int}                          every `#define HDY_NAME <integer expression>`
Rules: any `T*` is c_void_p, except `const char*` / `char*`, which is c_char_p; scalars by SCALARS; a `void` return is None.  The reader is strict:
whatever it cannot classify raises HdyError with the symbol and the offending text.  A half-understood header must stop the import instead of
shifting the arguments of a kernel launch.
"""
import ctypes
import functools
import os
import re
from collections import namedtuple

HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'hdyolo.h')
EXTENSION_NAMES = ('measure', 'spatial', 'outline', 'graph', 'texture')      # the extension headers, oldest first: _ext.py binds them, build.py watches them
# The extension headers of the passes over a slide's pixels.  A second tuple only because the tests of the five headers above pin that tuple and
# the sizes of its tables: _ext.py binds both alike (PIXEL_EXTENSIONS beside EXTENSIONS), and the two can be merged once those tests may change.
PIXEL_EXTENSION_NAMES = ('stain',)
SCALARS = {'int': ctypes.c_int, 'unsigned': ctypes.c_uint, 'long long': ctypes.c_longlong, 'unsigned long long': ctypes.c_ulonglong,
           'size_t': ctypes.c_size_t, 'float': ctypes.c_float, 'double': ctypes.c_double}
POINTEES = set(SCALARS) | {'void', 'char', 'unsigned char', 'unsigned short', 'uint16_t'}       # what a pointer may point at, beside a structure
Header = namedtuple('Header', 'functions params structs constants')
_INT = r'(0[xX][0-9a-fA-F]+|0|[1-9][0-9]*)(?:[uU]|[uU]?(?:ll|LL))?'


class HdyError(RuntimeError):
    pass


def extension_header(name):
    """the path of the extension header of that short name, beside include/hdyolo.h"""
    return os.path.join(os.path.dirname(HEADER_PATH), f'hdyolo_{name}.h')


def _ctype(symbol, text, structs):
    """(ctypes type, const) of a type written without a declarator: `const float*`, `unsigned long long`, `hdy_pack_desc*`"""
    words = ' '.join(re.sub(r'\bconst\b|\*', ' ', text).split())
    stars = text.count('*')
    if not re.fullmatch(r'[\w\s*]+', text) or words not in (POINTEES | set(structs) if stars else SCALARS):
        raise HdyError(f'include/hdyolo.h, {symbol}: unknown type {" ".join(text.split())!r}')
    ctype = SCALARS[words] if not stars else ctypes.c_char_p if (words, stars) == ('char', 1) else ctypes.c_void_p
    return ctype, re.match(r'\s*const\b', text) is not None


def _declared(symbol, text, structs):
    """(name, ctypes type, const) of one declaration `type name`; arrays, callbacks and nested structures are refused"""
    m = re.fullmatch(r'\s*([\w\s*]*[\s*])(\w+)\s*', text)
    if m is None:
        raise HdyError(f'include/hdyolo.h, {symbol}: cannot read the declaration {" ".join(text.split())!r}')
    return (m.group(2),) + _ctype(f'{symbol}, {m.group(2)}', m.group(1), structs)


def _constant(name, value):
    m = re.fullmatch(_INT, value)
    if m:
        return int(m.group(1), 0)
    m = re.fullmatch(rf'\(\s*{_INT}\s*<<\s*{_INT}\s*\)', value)
    if m:
        return int(m.group(1), 0) << int(m.group(2), 0)
    raise HdyError(f'include/hdyolo.h, {name}: {value!r} is not an integer expression this reader knows (n, 0xn, suffixes u / ull / LL, (a << b))')


def parse(text):
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    text = re.sub(r'//[^\n]*', ' ', text)
    text = re.sub(r'^[ \t]*#[ \t]*ifdef[ \t]+__cplusplus\b.*?^[ \t]*#[ \t]*endif\b', ' ', text, flags=re.S | re.M)      # the extern "C" braces
    constants = {name: _constant(name, value.strip())
                 for name, value in re.findall(r'^[ \t]*#[ \t]*define[ \t]+(HDY_\w+)(.*)$', text, flags=re.M)}
    text = re.sub(r'^[ \t]*#.*$', ' ', text, flags=re.M)
    structs = {}

    def struct(m):
        name, fields = m.group(2), []
        for stmt in filter(None, (s.strip() for s in m.group(1).split(';'))):
            first, *more = stmt.split(',')
            base = re.fullmatch(r'([\w\s]+?)\s*(\**\s*\w+)', first.strip())        # `const float *scale, *shift`: the base type serves every declarator
            if base is None:
                raise HdyError(f'include/hdyolo.h, {name}: cannot read the member {stmt!r}')
            for decl in [base.group(2)] + more:
                fields.append(_declared(name, base.group(1) + ' ' + decl, structs)[:2])
        structs[name] = type(name, (ctypes.Structure,), {'_fields_': fields, '__doc__': f'{name} (include/hdyolo.h)'})
        return ' '

    text = re.sub(r'\btypedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;', struct, text)
    functions, params = {}, {}
    for stmt in filter(None, (s.strip() for s in text.split(';'))):        # what is left: prototypes, one per statement
        m = re.fullmatch(r'([\w\s*]+?)\b(\w+)\s*\((.*)\)', stmt, flags=re.S)
        if m is None:
            raise HdyError(f'include/hdyolo.h: neither a prototype nor a `typedef struct {{ ... }} name;` of plain members: {" ".join(stmt.split())!r}')
        name, plist = m.group(2), m.group(3).strip()
        restype = None if m.group(1).strip() == 'void' else _ctype(name, m.group(1), structs)[0]
        decls = [] if plist == 'void' else [_declared(name, p, structs) for p in plist.split(',')]
        functions[name] = (restype, [d[1] for d in decls])
        params[name] = [(d[0], d[2]) for d in decls]
    return Header(functions, params, structs, constants)


@functools.lru_cache(maxsize=None)
def read(path=HEADER_PATH):
    """the parsed header (read once per process)"""
    if not os.path.exists(path):
        raise HdyError(f'{path} is missing: hd_yolo_amd derives its ctypes binding from the public header, which belongs beside the package')
    with open(path) as f:
        return parse(f.read())
