#!/usr/bin/env python3
"""Recorded kernel-selection answers of the host-side sizing queries (no GPU needed: the queries are pure host functions):

    python tests/golden/make_golden_dispatch.py          # writes dispatch_sweep.npz

  dispatch_sweep.npz   hdy_conv_stat_slabs and hdy_conv_dgrad_stat_slabs over SHAPES x SETTINGS, hdy_conv_wgrad_workspace_bytes over
                       SHAPES (default options; stem = 0 for every shape, stem = 1 for the C = 3 6x6/s2 shapes)

The table was recorded from the build of commit 219272b ("Add poison-scratch and repeat tests for conv, BN and seg kernel paths"), the
parent of the change that made one plan function per kernel family serve both the sizing query and the launch.  It is the record of
what that commit selected, so it is NEVER regenerated from a later build to make a test pass: a later build that answers differently
has changed which kernel (or which grid) serves a shape.  Regenerate only together with a deliberate selection change, from the
build that change is compared against, and say so in that commit.

    python tests/golden/make_golden_dispatch.py wgrad    # writes wgrad_sweep.npz

  wgrad_sweep.npz      hdy_conv_wgrad_workspace_bytes over SHAPES (stem = 0) and over a stem list of its own (wgrad_stem_shapes) under
                       WGRAD_SETTINGS: the first table sees the weight gradient at default options only, and only 2 of its 720 stem rows
                       notice the stem kernel

wgrad_sweep.npz was recorded from the build of commit 7a393fd ("Split the backward-list compiler into a builder and per-unit emitters"),
the parent of the change that gave the weight gradient one plan per kernel family, under the same rule: never regenerated to make a
test pass.

tests/test_dispatch_golden.py replays sweep() and wgrad_sweep() against the built library and requires every entry equal.
"""
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, 'dispatch_sweep.npz')

NS = (1, 2, 64)
HWS = ((8, 16), (20, 20), (24, 24), (32, 32), (40, 40), (64, 64), (80, 80), (160, 160), (320, 320), (37, 53))
CS = (3, 8, 16, 32, 48, 64, 96, 128, 192, 256, 384, 512, 1024)
KS = (16, 32, 40, 48, 64, 72, 96, 128, 192, 256, 512, 1024)
WINDOWS = ((1, 1, 0), (3, 1, 1), (3, 2, 1), (6, 2, 2), (5, 1, 2))       # (R = S, stride, pad)
DTYPES = (0, 1)                                                          # HDY_F32, HDY_BF16
# one option away from the defaults each; () = the defaults
SETTINGS = ((), ('HDY_NO_CONV3X3', 1), ('HDY_NO_CONV3X3_C128', 1), ('HDY_NO_CONV3X3S2', 1), ('HDY_NO_DEEP', 1), ('HDY_NO_STEM_KERNEL', 1),
            ('HDY_NO_BIG_TILES', 1), ('HDY_NO_CLASS_WALK', 1), ('HDY_NO_CONV3X3S2', 2), ('HDY_DEEP_BN', 128), ('HDY_DEEP_BN', 256),
            ('HDY_DEEP_ALL', 0), ('HDY_DEEP_MIN_TILES', 16), ('HDY_TILE_INTERLEAVE', 0))

# the weight gradient's own table: every family's switch and the generic kernel's two sizing options
WGRAD_OUT = os.path.join(HERE, 'wgrad_sweep.npz')
WGRAD_SETTINGS = ((), ('HDY_NO_WGRAD3X3', 1), ('HDY_NO_WGRAD_DEEP', 1), ('HDY_NO_STEM_WGRAD', 1), ('HDY_WGRAD_DEEP_KMIN', 256),
                  ('HDY_WGRAD_BLOCKS', 1024), ('HDY_WGRAD_TILE', 64), ('HDY_WGRAD_TILE', 4096))
WGRAD_STEM_HWS = ((64, 64), (64, 128), (128, 256), (256, 256), (640, 640), (96, 80))
WGRAD_STEM_KS = (16, 32, 48, 64, 96)


def shapes():
    """[n][10] int32: (N, H, W, C, K, R, S, stride, pad, dtype), the argument list of the two slab queries."""
    rows = [(n, h, w, c, k, r, r, s, p, dt) for n, (h, w), c, k, (r, s, p), dt in itertools.product(NS, HWS, CS, KS, WINDOWS, DTYPES)]
    return np.asarray(rows, dtype=np.int32)


def sweep(lib):
    """Answers of `lib` (the loaded ctypes library): fwd[setting][shape], dgrad[setting][shape] (int32), ws0[shape], ws1[stem shape] (int64)."""
    sh = [tuple(int(v) for v in row) for row in shapes()]
    fwd = np.zeros((len(SETTINGS), len(sh)), dtype=np.int32)
    dgrad = np.zeros_like(fwd)
    q_fwd, q_dgrad, q_ws = lib.hdy_conv_stat_slabs, lib.hdy_conv_dgrad_stat_slabs, lib.hdy_conv_wgrad_workspace_bytes
    for i, setting in enumerate(SETTINGS):
        prev = lib.hdy_set_option(setting[0].encode(), setting[1]) if setting else None
        try:
            fwd[i] = [q_fwd(*s) for s in sh]
            dgrad[i] = [q_dgrad(*s) for s in sh]
        finally:
            if setting:
                lib.hdy_set_option(setting[0].encode(), prev)
    ws0 = np.asarray([q_ws(*s, 0) for s in sh], dtype=np.int64)
    ws1 = np.asarray([q_ws(*s, 1) for s in sh if s[3] == 3 and s[5] == 6], dtype=np.int64)
    return {'fwd': fwd, 'dgrad': dgrad, 'ws0': ws0, 'ws1': ws1}


def wgrad_stem_shapes():
    """[n][10] int32 stem rows (C = 3, 6x6 / stride 2 / pad 2): image sides and widths on both sides of what the stem kernel takes."""
    rows = [(n, h, w, 3, k, 6, 6, 2, 2, dt) for n, (h, w), k, dt in itertools.product(NS, WGRAD_STEM_HWS, WGRAD_STEM_KS, DTYPES)]
    return np.asarray(rows, dtype=np.int32)


def wgrad_sweep(lib):
    """hdy_conv_wgrad_workspace_bytes of `lib` under WGRAD_SETTINGS: ws0[setting][shape] (stem = 0), ws1[setting][stem shape] (int64).  Row 0
    holds the answers at default options, every later row what its setting adds to them (mostly zeros: a third of the file size)."""
    sh = [tuple(int(v) for v in row) for row in shapes()]
    st = [tuple(int(v) for v in row) for row in wgrad_stem_shapes()]
    ws0 = np.zeros((len(WGRAD_SETTINGS), len(sh)), dtype=np.int64)
    ws1 = np.zeros((len(WGRAD_SETTINGS), len(st)), dtype=np.int64)
    q_ws = lib.hdy_conv_wgrad_workspace_bytes
    for i, setting in enumerate(WGRAD_SETTINGS):
        prev = lib.hdy_set_option(setting[0].encode(), setting[1]) if setting else None
        try:
            ws0[i] = [q_ws(*s, 0) for s in sh]
            ws1[i] = [q_ws(*s, 1) for s in st]
        finally:
            if setting:
                lib.hdy_set_option(setting[0].encode(), prev)
    ws0[1:] -= ws0[0]
    ws1[1:] -= ws1[0]
    return {'ws0': ws0, 'ws1': ws1}


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from hd_yolo_amd import _lib
    if 'wgrad' in sys.argv[1:]:
        got = wgrad_sweep(_lib.load())
        # the SHAPES grid itself is in dispatch_sweep.npz
        np.savez_compressed(WGRAD_OUT, stem_shapes=wgrad_stem_shapes(), settings=np.asarray(['='.join(map(str, s)) for s in WGRAD_SETTINGS]), **got)
        changed = [int((got['ws0'][i] != 0).sum() + (got['ws1'][i] != 0).sum()) for i in range(1, len(WGRAD_SETTINGS))]
        print(WGRAD_OUT, os.path.getsize(WGRAD_OUT), 'bytes; entries each setting changes against the defaults:', changed)
        sys.exit(0)
    got = sweep(_lib.load())
    np.savez_compressed(OUT, shapes=shapes(), settings=np.asarray(['='.join(map(str, s)) for s in SETTINGS]), **got)
    print(OUT, os.path.getsize(OUT), 'bytes;', len(np.unique(np.stack([got['fwd'], got['dgrad']], -1).reshape(-1, 2), axis=0)), 'distinct answer pairs')
