"""ctypes binding of the extension headers of libhdyolo_hip.so (include/hdyolo_<name>.h for every name of _header.EXTENSION_NAMES: measure,
spatial, outline, graph, texture; and of _header.PIXEL_EXTENSION_NAMES: stain).

include/hdyolo.h is the numbered ABI and _lib.py its binding; an extension header declares further entry points of the same library under a
revision of its own, read by the same reader (_header.read(path)) and bound here on the handle _lib.load() returns.  _lib.SIGNATURES,
_lib.CONSTANTS and HDY_ABI_VERSION know nothing of them.  No CPU fallback: a library without the symbols, or of another revision, raises.

EXTENSIONS maps an extension's short name to its tables; SIGNATURES, PARAMS and CONSTANTS are their unions.  A name belongs to one header:
the import fails when two of them, or one of them and include/hdyolo.h, declare the same function or constant.  PIXEL_EXTENSIONS,
PIXEL_SIGNATURES, PIXEL_PARAMS and PIXEL_CONSTANTS are the same tables for the headers of _header.PIXEL_EXTENSION_NAMES; load() binds both
and the names are disjoint over both.
"""
import os
from collections import namedtuple

from . import _header, _lib
from ._header import HdyError

# functions, params, constants: as _header.Header's; revision_fn returns the library's revision, revision_macro states the one bound here
Extension = namedtuple('Extension', 'header functions params constants revision_fn revision revision_macro')



def _table(names):
    """{short name: Extension} of the headers of `names`, in that order"""
    table = {}
    for name in names:
        path, macro = _header.extension_header(name), f'HDY_{name.upper()}_REVISION'
        h = _header.read(path)
        table[name] = Extension(path, h.functions, h.params, h.constants, f'hdy_{name}_revision', h.constants[macro], macro)
    return table


EXTENSIONS = _table(_header.EXTENSION_NAMES)
PIXEL_EXTENSIONS = _table(_header.PIXEL_EXTENSION_NAMES)      # why a second table: _header.PIXEL_EXTENSION_NAMES


def check_disjoint(extensions):
    """raise HdyError when a function or a constant is declared twice among include/hdyolo.h and the headers of `extensions`"""
    owner = dict.fromkeys((*_lib.SIGNATURES, *_lib.CONSTANTS), os.path.basename(_header.HEADER_PATH))
    for ext in extensions.values():
        for name in (*ext.functions, *ext.constants):
            if name in owner:
                raise HdyError(f'{name} is declared by include/{owner[name]} and by include/{os.path.basename(ext.header)}: a name belongs to one header')
            owner[name] = os.path.basename(ext.header)


check_disjoint(EXTENSIONS)
check_disjoint({**EXTENSIONS, **PIXEL_EXTENSIONS})
SIGNATURES = {n: v for e in EXTENSIONS.values() for n, v in e.functions.items()}
PARAMS = {n: v for e in EXTENSIONS.values() for n, v in e.params.items()}
CONSTANTS = {n: v for e in EXTENSIONS.values() for n, v in e.constants.items()}
PIXEL_SIGNATURES = {n: v for e in PIXEL_EXTENSIONS.values() for n, v in e.functions.items()}
PIXEL_PARAMS = {n: v for e in PIXEL_EXTENSIONS.values() for n, v in e.params.items()}
PIXEL_CONSTANTS = {n: v for e in PIXEL_EXTENSIONS.values() for n, v in e.constants.items()}

_bound = None


def load():
    """The library handle of _lib.load() with the extensions' entry points bound (once)."""
    global _bound
    lib = _lib.load()
    if _bound is not lib:
        rebuild = 'rebuild with `python -m hd_yolo_amd.build --force`'
        for ext in (*EXTENSIONS.values(), *PIXEL_EXTENSIONS.values()):
            header = os.path.basename(ext.header)
            for name, (res, args) in ext.functions.items():
                fn = getattr(lib, name, None)
                if fn is None:
                    raise HdyError(f'{_lib.LIB_PATH} does not export {name} (include/{header}): it was built before the extension header '
                                   f'existed; {rebuild}')
                fn.restype, fn.argtypes = res, args
            got = getattr(lib, ext.revision_fn)()
            if got != ext.revision:
                raise HdyError(f'{_lib.LIB_PATH} was built for revision {got} of include/{header}, this binding is written for '
                               f'{ext.revision} ({ext.revision_macro}): {rebuild}')
        _bound = lib
    return lib


def call(name, *args):
    """Call an int-returning entry point of an extension; raise HdyError(hdy_last_error()) on a non-zero status."""
    lib = load()
    rc = getattr(lib, name)(*args)
    if rc != 0:
        raise HdyError(f'{name} failed (status {rc}): {lib.hdy_last_error().decode()}')
