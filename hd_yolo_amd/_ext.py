"""ctypes binding of the extension headers of libhdyolo_hip.so (include/hdyolo_measure.h, include/hdyolo_spatial.h, include/hdyolo_outline.h,
include/hdyolo_graph.h).

include/hdyolo.h is the numbered ABI and _lib.py its binding; an extension header declares further entry points of the same library under a
revision of its own, read by the same reader (_header.read(path)) and bound here on the handle _lib.load() returns.  _lib.SIGNATURES,
_lib.CONSTANTS and HDY_ABI_VERSION know nothing of them.  No CPU fallback: a library without the symbols, or of another revision, raises.

MEASURE_HEADER, SIGNATURES, PARAMS and CONSTANTS are the tables of hdyolo_measure.h, the first extension header; hdyolo_spatial.h has
SPATIAL_HEADER, SPATIAL_SIGNATURES, SPATIAL_PARAMS and SPATIAL_CONSTANTS, hdyolo_outline.h the same four under OUTLINE_, hdyolo_graph.h under GRAPH_.
"""
import os

from . import _header, _lib
from ._header import HdyError

MEASURE_HEADER = os.path.join(os.path.dirname(_header.HEADER_PATH), 'hdyolo_measure.h')
_M = _header.read(MEASURE_HEADER)
SIGNATURES = _M.functions         # name -> (restype, [argtypes]) of every function include/hdyolo_measure.h declares
PARAMS = _M.params
CONSTANTS = _M.constants
MEASURE_REVISION, MEASURE_COLS, MEASURE_MAX_SIDE = (CONSTANTS['HDY_MEASURE_' + n] for n in ('REVISION', 'COLS', 'MAX_SIDE'))

SPATIAL_HEADER = os.path.join(os.path.dirname(_header.HEADER_PATH), 'hdyolo_spatial.h')
_S = _header.read(SPATIAL_HEADER)
SPATIAL_SIGNATURES = _S.functions
SPATIAL_PARAMS = _S.params
SPATIAL_CONSTANTS = _S.constants
SPATIAL_REVISION, SPATIAL_SUBPIXEL, SPATIAL_MAX_CLASSES, SPATIAL_MAX_RADII, SPATIAL_MAX_COORD, SPATIAL_MAX_CELLS = (
    SPATIAL_CONSTANTS['HDY_SPATIAL_' + n] for n in ('REVISION', 'SUBPIXEL', 'MAX_CLASSES', 'MAX_RADII', 'MAX_COORD', 'MAX_CELLS'))

OUTLINE_HEADER = os.path.join(os.path.dirname(_header.HEADER_PATH), 'hdyolo_outline.h')
_O = _header.read(OUTLINE_HEADER)
OUTLINE_SIGNATURES = _O.functions
OUTLINE_PARAMS = _O.params
OUTLINE_CONSTANTS = _O.constants
OUTLINE_REVISION, OUTLINE_MAX_SIDE, OUTLINE_MAX_WINDOW = (OUTLINE_CONSTANTS['HDY_OUTLINE_' + n] for n in ('REVISION', 'MAX_SIDE', 'MAX_WINDOW'))

GRAPH_HEADER = os.path.join(os.path.dirname(_header.HEADER_PATH), 'hdyolo_graph.h')
_G = _header.read(GRAPH_HEADER)
GRAPH_SIGNATURES = _G.functions
GRAPH_PARAMS = _G.params
GRAPH_CONSTANTS = _G.constants
GRAPH_REVISION, GRAPH_MAX_K, GRAPH_MAX_RINGS = (GRAPH_CONSTANTS['HDY_GRAPH_' + n] for n in ('REVISION', 'MAX_K', 'MAX_RINGS'))

# header file name -> (signatures, the function that returns the library's revision, the revision this binding is written for, its macro)
_EXTENSIONS = {'hdyolo_measure.h': (SIGNATURES, 'hdy_measure_revision', MEASURE_REVISION, 'HDY_MEASURE_REVISION'),
               'hdyolo_spatial.h': (SPATIAL_SIGNATURES, 'hdy_spatial_revision', SPATIAL_REVISION, 'HDY_SPATIAL_REVISION'),
               'hdyolo_outline.h': (OUTLINE_SIGNATURES, 'hdy_outline_revision', OUTLINE_REVISION, 'HDY_OUTLINE_REVISION'),
               'hdyolo_graph.h': (GRAPH_SIGNATURES, 'hdy_graph_revision', GRAPH_REVISION, 'HDY_GRAPH_REVISION')}

_bound = None


def load():
    """The library handle of _lib.load() with the extensions' entry points bound (once)."""
    global _bound
    lib = _lib.load()
    if _bound is not lib:
        rebuild = 'rebuild with `python -m hd_yolo_amd.build --force`'
        for header, (signatures, revision_fn, revision, macro) in _EXTENSIONS.items():
            for name, (res, args) in signatures.items():
                fn = getattr(lib, name, None)
                if fn is None:
                    raise HdyError(f'{_lib.LIB_PATH} does not export {name} (include/{header}): it was built before the extension header '
                                   f'existed; {rebuild}')
                fn.restype, fn.argtypes = res, args
            got = getattr(lib, revision_fn)()
            if got != revision:
                raise HdyError(f'{_lib.LIB_PATH} was built for revision {got} of include/{header}, this binding is written for '
                               f'{revision} ({macro}): {rebuild}')
        _bound = lib
    return lib


def call(name, *args):
    """Call an int-returning entry point of an extension; raise HdyError(hdy_last_error()) on a non-zero status."""
    lib = load()
    rc = getattr(lib, name)(*args)
    if rc != 0:
        raise HdyError(f'{name} failed (status {rc}): {lib.hdy_last_error().decode()}')
