"""ctypes binding of libhdyolo_hip.so, derived from include/hdyolo.h.

Signatures, structures and constants are read from the header (_header.py) when this module is imported: adding an entry point is an edit of the
header alone.  The product path has no CPU fallback: if the library is missing or a call fails this module raises.
"""
import ctypes
import os

import torch  # noqa: F401  -- must come first: the library has to bind to the HIP runtime torch already loaded,
#                              otherwise a second libamdhip64 gets mapped and sees no device

from . import _header
from ._header import HdyError  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
# HDY_LIB: load another build of the same ABI (kernel A/B experiments); it must still sit under csrc/build/
LIB_PATH = os.path.join(_HERE, 'csrc', 'build', os.path.basename(os.environ.get('HDY_LIB', 'libhdyolo_hip.so')))

_H = _header.read()
SIGNATURES = _H.functions         # name -> (restype, [argtypes]) of every function include/hdyolo.h declares
PARAMS = _H.params                # name -> [(parameter name, const)], position by position beside SIGNATURES[name][1]
STRUCTS = _H.structs              # typedef name -> the structure as a ctypes class
CONSTANTS = _H.constants          # HDY_NAME -> int, every integer macro of the header

ABI_VERSION = CONSTANTS['HDY_ABI_VERSION']      # load() refuses a library built from another revision of the header
OK, EINVAL, EUNSUPPORTED = 0, -1, -2      # status codes (the header's return-value convention); positive = hipError_t
F32, BF16 = (CONSTANTS['HDY_' + n] for n in ('F32', 'BF16'))
PACK_FWD, PACK_DGRAD, PACK_STEM = (CONSTANTS['HDY_PACK_' + n] for n in ('FWD', 'DGRAD', 'STEM'))
ACT_NONE, ACT_SILU, ACT_RELU = (CONSTANTS['HDY_ACT_' + n] for n in ('NONE', 'SILU', 'RELU'))
OPT_SGD, OPT_ADAM, OPT_ADAMW = (CONSTANTS['HDY_OPT_' + n] for n in ('SGD', 'ADAM', 'ADAMW'))
OPT_MAX_SLOTS, OPT_HYPER = CONSTANTS['HDY_OPT_MAX_SLOTS'], CONSTANTS['HDY_OPT_HYPER']

PackDesc, BnEvalDesc = STRUCTS['hdy_pack_desc'], STRUCTS['hdy_bn_eval_desc']
OptDesc, StatReq, RoiLevel = STRUCTS['hdy_opt_desc'], STRUCTS['hdy_stat_req'], STRUCTS['hdy_roi_level']


def device_table(descs, device):
    """A ctypes array, or a sequence of structures, as a uint8 tensor on `device`: the descriptor table a batched entry point replays."""
    raw = bytes(descs) if isinstance(descs, ctypes.Array) else b''.join(bytes(d) for d in descs)
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(device)


_lib = None


def load():
    """Load the shared library (once).  Raises HdyError with build instructions if it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HdyError(f'{LIB_PATH} is missing: run `python -m hd_yolo_amd.build` (hipcc, gfx950). '
                           'hd_yolo_amd has no CPU fallback.')
        lib = ctypes.CDLL(LIB_PATH)
        lib.hdy_version.restype, lib.hdy_version.argtypes = SIGNATURES['hdy_version']
        got = lib.hdy_version()
        if got != ABI_VERSION:
            # SIGNATURES is the header's parameter lists: a library built before the header was edited would receive shifted arguments instead of an error
            raise HdyError(f'{LIB_PATH} was built for ABI revision {got}, this binding is written for {ABI_VERSION} (include/hdyolo.h HDY_ABI_VERSION): '
                           'rebuild with `python -m hd_yolo_amd.build --force`')
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        _lib = lib
    return _lib


def call(name, *args):
    """Call an int-returning entry point; raise HdyError(hdy_last_error()) on a non-zero status."""
    lib = load()
    rc = getattr(lib, name)(*args)
    if rc != 0:
        raise HdyError(f'{name} failed (status {rc}): {lib.hdy_last_error().decode()}')


def query(name, *args):
    return getattr(load(), name)(*args)


# ---- kernel selection: switches and the dispatch log (include/hdyolo.h) -----------------------------------------------------------
class option:
    """`with _lib.option('HDY_NO_CONV3X3', 1): ...` — a process-wide switch for the duration of the block (set it BEFORE sizing buffers or
    building plans: the switches also steer the slab / workspace queries)."""

    def __init__(self, name, value):
        self.name, self.value = name.encode(), int(value)

    def __enter__(self):
        self.prev = load().hdy_set_option(self.name, self.value)
        if self.prev < 0 and load().hdy_get_option(self.name) != self.value:
            raise HdyError(f'unknown option {self.name.decode()}')
        return self

    def __exit__(self, *exc):
        load().hdy_set_option(self.name, self.prev)
        return False


def dispatch_log(reset=False):
    """kernel families picked (by any thread) since the last reset, in launch order"""
    lib = load()
    names = [n for n in lib.hdy_dispatch_log().decode().split(';') if n]
    if reset:
        lib.hdy_dispatch_log_reset()
    return names
