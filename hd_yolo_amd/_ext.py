"""ctypes binding of the extension headers of libhdyolo_hip.so (include/hdyolo_measure.h).

include/hdyolo.h is the numbered ABI and _lib.py its binding; an extension header declares further entry points of the same library under a
revision of its own, read by the same reader (_header.read(path)) and bound here on the handle _lib.load() returns.  _lib.SIGNATURES,
_lib.CONSTANTS and HDY_ABI_VERSION know nothing of them.  No CPU fallback: a library without the symbols, or of another revision, raises.
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

_bound = None


def load():
    """The library handle of _lib.load() with the extension's entry points bound (once)."""
    global _bound
    lib = _lib.load()
    if _bound is not lib:
        rebuild = 'rebuild with `python -m hd_yolo_amd.build --force`'
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name, None)
            if fn is None:
                raise HdyError(f'{_lib.LIB_PATH} does not export {name} (include/hdyolo_measure.h): it was built before the extension header '
                               f'existed; {rebuild}')
            fn.restype, fn.argtypes = res, args
        got = lib.hdy_measure_revision()
        if got != MEASURE_REVISION:
            raise HdyError(f'{_lib.LIB_PATH} was built for revision {got} of include/hdyolo_measure.h, this binding is written for '
                           f'{MEASURE_REVISION} (HDY_MEASURE_REVISION): {rebuild}')
        _bound = lib
    return lib


def call(name, *args):
    """Call an int-returning entry point of the extension; raise HdyError(hdy_last_error()) on a non-zero status."""
    lib = load()
    rc = getattr(lib, name)(*args)
    if rc != 0:
        raise HdyError(f'{name} failed (status {rc}): {lib.hdy_last_error().decode()}')
