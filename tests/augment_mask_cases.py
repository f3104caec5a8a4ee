"""The hand-made masked tile bank and the parametrised cases that tests/test_augment_masks_host.py (CPU) and tests/test_gpu_augment_masks.py
share (a helper, not a test).  The restatement's result of a case is computed once per process."""
import functools

import numpy as np

import augment_mask_ref as mref
from hd_yolo_amd import augment

BG = 0xFFFF
H, W = 40, 56                                   # tiles with H != W
B, K, PATCH, SIZE = 3, 2, 48, 64
CROPS = ((16, 16), (0, 32), (32, 5))            # k * patch - img_size = 32: every offset in [0, 32] puts the image across all four cells
MILD = dict(degrees=10.0, shear=2.0, scale=0.2)
STRONG = dict(degrees=45.0, shear=20.0, scale=0.5)
PARITY_CASES = {f'{"persp" if p else "affine"}_{"strong" if s else "mild"}': (p, s) for p in (False, True) for s in (False, True)}
SEEDS = {'affine_mild': 9, 'affine_strong': 2, 'persp_mild': 17, 'persp_strong': 8}       # chosen on the CPU: see the counts asserted on them


def disc(m, idx, cx, cy, rx, ry):
    ys, xs = np.mgrid[0:H, 0:W]
    m[((xs + 0.5 - cx) / rx) ** 2 + ((ys + 0.5 - cy) / ry) ** 2 <= 1.0] = idx


def hand_bank():
    """4 tiles of 40 x 56 with 2 .. 6 objects each: plain discs, an object with no pixels, one of fewer than 25 pixels spread over a 13 x 13
    extent, one touching the tile edge, one half overwritten by its neighbour, one whose pixels sit in a corner of a much larger box"""
    rng = np.random.default_rng(7)
    tiles = rng.integers(0, 256, (4, H, W, 3), dtype=np.uint8)
    inst = np.full((4, H, W), BG, np.uint16)
    boxes, labels, offsets = [], [], [0]

    def add(t, objs):
        for idx, (box, paint) in enumerate(objs):
            if paint is not None:
                paint(inst[t], idx)
            boxes.append(box)
            labels.append(1 + (len(boxes) % 2))
        offsets.append(offsets[-1] + len(objs))

    def sparse(m, idx):                          # 7 pixels on a diagonal: 13 x 13 extent, fewer than 25 pixels at any scale below 1.8
        for i in range(7):
            m[20 + 2 * i, 36 + 2 * i] = idx

    def corner(m, idx):                          # a disc of 14 pixels across in the corner of a 56 x 39 box: area ratio 0.09 at any rotation
        disc(m, idx, 7, 7, 7, 7)

    def rect(x1, y1, x2, y2):
        def paint(m, idx):
            m[y1:y2, x1:x2] = idx
        return paint

    add(0, [((4.5, 6.25, 24.5, 26.25), lambda m, i: disc(m, i, 14.5, 16.25, 10, 10)),
            ((30.0, 4.0, 50.0, 18.0), None),                                              # no pixels: an object without a mask
            ((36.0, 20.0, 49.0, 33.0), sparse)])
    add(1, [((0.0, 8.0, 18.0, 30.0), rect(0, 8, 18, 30)),                                 # touches the tile's left edge
            ((22.0, 2.0, 42.0, 20.0), rect(22, 2, 42, 20)),
            ((32.0, 10.0, 54.0, 32.0), rect(32, 10, 54, 32)),                             # overwrites half of its neighbour
            ((4.0, 30.5, 20.0, 40.0), lambda m, i: disc(m, i, 12, 35.25, 8, 4.75))])      # touches the bottom edge
    add(2, [((0.0, 0.0, 56.0, 39.0), corner),
            ((28.3, 14.2, 47.9, 33.6), lambda m, i: disc(m, i, 38.1, 23.9, 9.8, 9.7))])
    add(3, [((2.0, 2.0, 20.0, 18.0), lambda m, i: disc(m, i, 11, 10, 9, 8)),
            ((18.0, 18.0, 40.0, 38.0), lambda m, i: disc(m, i, 29, 28, 11, 10)),
            ((38.0, 2.0, 56.0, 16.0), rect(38, 2, 56, 16)),                               # touches the right edge
            ((24.0, 1.0, 36.0, 13.0), lambda m, i: disc(m, i, 30, 7, 6, 6)),
            ((42.0, 20.0, 55.0, 38.0), None),
            ((1.0, 22.0, 15.0, 39.0), rect(1, 22, 15, 39))])
    return augment.TileBank(tiles, np.asarray(boxes, np.float32), np.asarray(labels, np.int64), np.asarray(offsets, np.int64), inst)


def make_hyp(k, patch, size, perspective=0.0, **kw):
    hyp = dict(degrees=10.0, translate=0.1, scale=0.2, shear=2.0, perspective=perspective, hsv_h=0.0, hsv_s=0.0, hsv_v=0.0, fliplr=0.5,
               flipud=0.5, transpose=0.5, cval=114, k_mosaic=k, patch_size=patch, img_size=size)
    hyp.update(kw)
    return hyp


@functools.lru_cache(maxsize=None)
def parity_case(name):
    """-> dict(bank, tab, rec, written, rows, stats) of one parametrised case: 3 images of 64 px from 2 x 2 cells of 48 px, all eight flip
    combinations over the twelve cells, crop offsets that put every image across four cells"""
    persp, strong = PARITY_CASES[name]
    bank = hand_bank()
    rng = np.random.default_rng(SEEDS[name])
    hyp = make_hyp(K, PATCH, SIZE, 0.002 if persp else 0.0, **(STRONG if strong else MILD))
    p = augment.draw_params(rng, hyp, B, bank.n)
    cells = np.arange(B * K * K).reshape(B, K * K)
    combo = (cells + np.arange(B)[:, None]) % 8
    p['hflip'], p['vflip'], p['transpose'] = (combo & 1) > 0, (combo & 2) > 0, (combo & 4) > 0
    p['src'] = (cells + SEEDS[name]) % bank.n                    # every tile three times
    p['crop'] = np.asarray(CROPS, np.int64)
    tab = augment.cell_tables(p, (H, W))
    stats = {}
    rec, written, rows = mref.augment_masks_ref(bank, tab.cells, tab.crop, PATCH, K, SIZE, stats=stats)
    return {'bank': bank, 'tab': tab, 'rec': rec, 'written': written, 'rows': rows, 'stats': stats, 'pitch': bank.max_per_tile}


def total_stats():
    tot = {}
    for name in PARITY_CASES:
        for key, v in parity_case(name)['stats'].items():
            tot[key] = tot.get(key, 0) + v
    return tot
