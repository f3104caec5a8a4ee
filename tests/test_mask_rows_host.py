"""Host-side argument checks of hdy_roi_align_levels_fwd and hdy_mask_rows (csrc/roi.hip): every refusal is decided before a launch, so it
can be asked for on a machine without a GPU with made-up device addresses.  No compute calls."""
import ctypes
import os
import re

import pytest

from hd_yolo_amd import _lib, build, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000      # a 16-byte aligned non-NULL "device pointer": nothing below may dereference it or launch


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


def level_table(nl, feat=FAKE, C=32):
    table = (ops._RoiLevel * max(nl, 1))()
    for l in range(max(nl, 1)):
        table[l] = ops._RoiLevel(feat, 16 >> min(l, 3), 16 >> min(l, 3), C, 1.0 / (8 << l))
    return table


def levels_call(lib, table=None, nl=3, C=32, boxes=FAKE, level=FAKE, nex=1, n_keep=FAKE, B=3, max_det=8, P=14, S=2, aligned=0, out=FAKE, out_rows=11,
                dtype=_lib.F32, null_table=False):
    table = level_table(nl, C=C) if table is None else table
    tp = None if null_table else ctypes.cast(table, ctypes.c_void_p)
    return lib.hdy_roi_align_levels_fwd(tp, nl, C, boxes, level, nex, n_keep, B, max_det, P, S, aligned, out, out_rows, dtype, None)


def test_revision_15_in_header_binding_and_library(lib):
    header = open(os.path.join(ROOT, 'include', 'hdyolo.h')).read()
    assert int(re.search(r'#define\s+HDY_ABI_VERSION\s+(\d+)', header).group(1)) == 15
    assert _lib.ABI_VERSION == 15 and lib.hdy_version() == 15
    for name in ('hdy_roi_align_levels_fwd', 'hdy_mask_rows'):
        assert name in _lib.SIGNATURES and hasattr(lib, name) and lib.hdy_exec_op(name.encode()) >= 0
    assert ctypes.sizeof(ops._RoiLevel) == 24       # hdy_roi_level: pointer, three ints, one float


def test_roi_align_levels_refuses_before_a_launch(lib):
    E = _lib.EINVAL
    assert levels_call(lib, null_table=True) == E and b'null' in lib.hdy_last_error()
    for name in ('boxes', 'level', 'n_keep', 'out'):
        assert levels_call(lib, **{name: None}) == E and b'null' in lib.hdy_last_error(), name
    assert levels_call(lib, table=level_table(3, feat=None)) == E and b'level 0' in lib.hdy_last_error()      # a null map inside the table
    assert levels_call(lib, nl=0) == E and b'0 levels' in lib.hdy_last_error()
    assert levels_call(lib, nl=9, table=level_table(9)) == E and b'9 levels' in lib.hdy_last_error()
    assert levels_call(lib, B=0) == E
    assert levels_call(lib, B=1025) == E and b'1025' in lib.hdy_last_error()
    assert levels_call(lib, C=12, dtype=_lib.BF16) == E and b'C = 12' in lib.hdy_last_error()             # 8 bf16 channels per vector
    assert levels_call(lib, C=12, dtype=_lib.F32, out_rows=0) == _lib.OK                                 # ... 12 is three fp32 vectors
    assert levels_call(lib, C=6, dtype=_lib.F32) == E
    assert levels_call(lib, P=0) == E and levels_call(lib, max_det=0) == E and levels_call(lib, out_rows=-1) == E and levels_call(lib, nex=0) == E
    assert levels_call(lib, out=FAKE + 4) == E and b'aligned' in lib.hdy_last_error()
    pitched = level_table(3)
    pitched[1].ldf = 16                                                                                   # a pitch below C
    assert levels_call(lib, table=pitched) == E and b'level 1' in lib.hdy_last_error()


def test_roi_align_levels_with_no_rows_is_ok(lib):
    assert levels_call(lib, out_rows=0) == _lib.OK
    assert levels_call(lib, out_rows=0, dtype=_lib.BF16, nl=8, table=level_table(8), B=1024) == _lib.OK


def rows_call(lib, vals=FAKE, ldv=8, K=3, labels=FAKE, table=FAKE, host=None, n_idx=4, R=5, M=28, out=FAKE, out_elems=None):
    arr = None if host is None else (ctypes.c_int * len(host))(*host)
    hp = None if arr is None else ctypes.cast(arr, ctypes.c_void_p)
    return lib.hdy_mask_rows(vals, ldv, K, labels, table, hp, n_idx, R, M, out, R * M * M if out_elems is None else out_elems, None)


def test_mask_rows_refuses_before_a_launch(lib):
    E = _lib.EINVAL
    for name in ('vals', 'labels', 'table', 'out'):
        assert rows_call(lib, **{name: None}) == E and b'null' in lib.hdy_last_error(), name
    assert rows_call(lib, out_elems=5 * 28 * 28 - 1) == E and b'out holds' in lib.hdy_last_error()
    assert rows_call(lib, out_elems=5 * 28 * 28 + 1) == E
    assert rows_call(lib, ldv=2) == E and rows_call(lib, K=0) == E and rows_call(lib, n_idx=0) == E and rows_call(lib, M=0) == E and rows_call(lib, R=-1, out_elems=0) == E
    assert rows_call(lib, host=[2, -1, 0, 3]) == E and b'mask_indices[3] = 3' in lib.hdy_last_error()     # idx >= K in a host-visible table
    assert rows_call(lib, R=0, host=[2, -1, 0, 1]) == _lib.OK                                            # a valid table, no rows: nothing to launch
    assert rows_call(lib, R=0) == _lib.OK
