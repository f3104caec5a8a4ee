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

tests/test_dispatch_golden.py replays sweep() against the built library and requires every entry equal.
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


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from hd_yolo_amd import _lib
    got = sweep(_lib.load())
    np.savez_compressed(OUT, shapes=shapes(), settings=np.asarray(['='.join(map(str, s)) for s in SETTINGS]), **got)
    print(OUT, os.path.getsize(OUT), 'bytes;', len(np.unique(np.stack([got['fwd'], got['dgrad']], -1).reshape(-1, 2), axis=0)), 'distinct answer pairs')
