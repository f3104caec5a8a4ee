"""Host side of the mask paste (csrc/paste.hip), no GPU: the numpy restatement of its arithmetic (tests/paste_ref.py) against torch's own
bilinear resize on the CPU, the box expansion with truncation toward zero, known answers derived by hand, and the ABI surface of the three
entry points (invalid calls answered by status and message before anything is dereferenced or launched)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import paste_ref as ref
from hd_yolo_amd import _lib, build

f32 = np.float32


def test_restatement_resize_equals_torch_bilinear_on_the_cpu():
    """paste_ref.resize against F.interpolate(mode='bilinear', align_corners=False) on the CPU: 400 seeded ellipse patches (P = 30) resized to
    h, w in 1..89, plus the fixed sizes.  The two evaluate the same four rounded steps, torch's vectorised kernel in another association in
    places.  Measured with this restatement: max |diff| 4.47e-7 over 774 091 pixels, no threshold flip.  The bound is twice the measured
    value, 8.94e-7, inside 1e-6 = 8 ulp at 1.0 for four rounded steps; no pixel may change side at the 0.5 threshold."""
    rng = np.random.default_rng(20240611)
    sizes = [(int(rng.integers(1, 90)), int(rng.integers(1, 90))) for _ in range(400)]
    sizes += [(1, 1), (30, 30), (60, 60), (640, 3), (2, 700), (29, 31)]
    worst, flips, pixels = 0.0, 0, 0
    for h, w in sizes:
        patch = ref.ellipse_patch(rng)
        want = F.interpolate(torch.from_numpy(patch)[None, None], size=(h, w), mode='bilinear', align_corners=False)[0, 0].numpy()
        got = ref.resize(patch, h, w)
        assert got.shape == want.shape == (h, w) and got.dtype == f32
        worst = max(worst, float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max()))
        flips += int(((got >= f32(0.5)) != (want >= f32(0.5))).sum())
        pixels += h * w
    print(f'resize vs torch: max |diff| {worst:.3e}, threshold flips {flips}, pixels {pixels}')
    assert worst <= 8.94e-7 <= 1e-6
    assert flips == 0


def test_box_expansion_truncates_toward_zero():
    boxes = np.array([[10.2, 5.7, 33.9, 40.1], [-3.5, -2.2, 8.0, 9.9]], dtype=f32)
    ib, ok = ref.integer_boxes(boxes, 28, 1)
    assert ok.all()
    assert ib.tolist() == [[9, 4, 34, 41], [-3, -2, 8, 10]]
    # the same expansion through torch's own fp32 arithmetic and int64 conversion (torchvision's expand_boxes followed by .to(int64))
    b = torch.from_numpy(boxes)
    scale = float(30) / 28
    hw, hh = (b[:, 2] - b[:, 0]) * 0.5 * scale, (b[:, 3] - b[:, 1]) * 0.5 * scale
    xc, yc = (b[:, 2] + b[:, 0]) * 0.5, (b[:, 3] + b[:, 1]) * 0.5
    assert torch.stack([xc - hw, yc - hh, xc + hw, yc + hh], 1).to(torch.int64).tolist() == ib.tolist()
    # floor would give -4, -3 on the negative side
    assert ref.integer_boxes(np.array([[np.nan, 0, 1, 1], [0, 0, np.inf, 1], [0, 0, 3e9, 1]], dtype=f32), 28, 1)[1].tolist() == [False] * 3


def test_all_ones_patch_without_padding_fills_its_integer_box():
    """padding 0: scale = 1, the box [10.5, 5.5, 33.5, 40.5] is its own expansion and truncates to columns 10..33, rows 5..40.  Every
    interpolated value of an all-ones patch is l0 + l1 with l0 = fl(1 - l1), which rounds back to exactly 1."""
    ones = np.ones((1, 28, 28), dtype=f32)
    box = np.array([[10.5, 5.5, 33.5, 40.5]], dtype=f32)
    want = np.zeros((48, 40), dtype=f32)
    want[5:41, 10:34] = 1
    dense = ref.paste_masks(ones, box, (48, 40), padding=0)
    assert dense.shape == (1, 48, 40) and np.array_equal(dense[0], want)
    lm = ref.label_map(ones, box, (0, 0, 40, 48), 0.5, padding=0)
    assert np.array_equal(lm, np.where(want > 0, 0, -1))
    assert ref.areas(lm, 1).tolist() == [36 * 24]


def test_border_ramp_with_padding_decides_the_edge_pixels():
    """padding 1, M = 28: P = 30, the all-ones mask framed by one ring of zeros.  The box [12.5, 12.5, 68, 68] expands about its centre 40.25 by
    30 / 28 to [10.51.., 69.98..] and truncates to 10..69: 60 pixels, sc = 30 / 60 = 0.5, s(d) = 0.5 d - 0.25.
      d = 0: s = 0 (clamped)           -> patch[0] = 0
      d = 1: s = 0.25: i0 = 0, l1 = .25 -> 0.25            (< 0.5)
      d = 2: s = 0.75: i0 = 0, l1 = .75 -> 0.75            (>= 0.5)
      d = 57: s = 28.25: i0 = 28, l1 = .25 -> 0.75;  d = 58: s = 28.75 -> 0.25;  d = 59: s = 29.25: i0 = i1 = 29 -> 0
    so offsets 2..57 pass along each axis: the label covers canvas 12..67 in both directions, 56 x 56 pixels."""
    ones = np.ones((1, 28, 28), dtype=f32)
    box = np.array([[12.5, 12.5, 68.0, 68.0]], dtype=f32)
    assert ref.integer_boxes(box, 28, 1)[0].tolist() == [[10, 10, 69, 69]]
    dense = ref.paste_masks(ones, box, (80, 80), padding=1)[0]
    ramp = np.zeros(60, dtype=f32)
    ramp[1], ramp[2:58], ramp[58] = 0.25, 1.0, 0.25
    ramp[2], ramp[57] = 0.75, 0.75
    want = np.zeros((80, 80), dtype=f32)
    want[10:70, 10:70] = ramp[:, None] * ramp[None, :]
    assert np.array_equal(dense, want)
    lm = ref.label_map(ones, box, (0, 0, 80, 80), 0.5, padding=1)
    owned = np.full((80, 80), -1, dtype=np.int32)
    owned[12:68, 12:68] = 0
    # 0.75 * 0.75 = 0.5625 >= 0.5 (the corners pass), 0.75 * 0.25 does not
    assert np.array_equal(lm, owned) and ref.areas(lm, 1).tolist() == [56 * 56]
    # at threshold 0.2 the 0.25 ring joins where its partner is 1 (0.25 * 1) but not at 0.25 * 0.75 = 0.1875
    lm2 = ref.label_map(ones, box, (0, 0, 80, 80), 0.2, padding=1)
    assert int((lm2 == 0).sum()) == 56 * 56 + 4 * 54


def test_outside_and_degenerate_boxes():
    ones = np.ones((3, 28, 28), dtype=f32)
    boxes = np.array([[100.5, 100.5, 120.5, 130.5],       # wholly outside the 40 x 32 canvas
                      [-50.5, -60.5, -10.5, -20.5],        # wholly outside on the negative side
                      [10.0, 20.0, 9.2, 19.2]], dtype=f32)  # degenerate: x2 < x1, y2 < y1
    # the degenerate box: half sizes -0.4 * (30 / 28) = -0.43, centre 9.6 / 19.6: expanded [10.03, 20.03, 9.17, 19.17] -> integers [10, 20, 9, 19],
    # w = h = max(9 - 10 + 1, 1) = 1; the 30 x 30 patch resized to 1 x 1 reads s = 30 * 0.5 - 0.5 = 14.5: the all-ones interior -> 1 at (10, 20)
    assert ref.integer_boxes(boxes, 28, 1)[0][2].tolist() == [10, 20, 9, 19]
    dense = ref.paste_masks(ones, boxes, (32, 40), padding=1)
    assert not dense[0].any() and not dense[1].any()
    want = np.zeros((32, 40), dtype=f32)
    want[20, 10] = 1
    assert np.array_equal(dense[2], want)
    lm = ref.label_map(ones, boxes, (0, 0, 40, 32), 0.5, padding=1)
    assert ref.areas(lm, 3).tolist() == [0, 0, 1] and lm[20, 10] == 2 and int((lm >= 0).sum()) == 1


def test_the_lower_row_owns_an_overlap():
    """two all-ones masks, padding 0: [2.5, 2.5, 10.5, 10.5] -> 2..10 (81 pixels) and [6.5, 6.5, 14.5, 14.5] -> 6..14 (81 pixels); they share
    6..10 in both directions (25 pixels), which row 0 owns: areas 81 and 56.  With the rows swapped the other one owns them."""
    ones = np.ones((2, 28, 28), dtype=f32)
    boxes = np.array([[2.5, 2.5, 10.5, 10.5], [6.5, 6.5, 14.5, 14.5]], dtype=f32)
    lm = ref.label_map(ones, boxes, (0, 0, 20, 20), 0.5, padding=0)
    assert (lm[6:11, 6:11] == 0).all() and ref.areas(lm, 2).tolist() == [81, 56]
    lm = ref.label_map(ones, boxes[::-1], (0, 0, 20, 20), 0.5, padding=0)
    assert (lm[6:11, 6:11] == 0).all() and (lm[2:6, 2:6] == 1).all() and ref.areas(lm, 2).tolist() == [81, 56]
    # a window cuts the same picture: columns 5..12, rows 4..9 of the canvas
    win = ref.label_map(ones, boxes, (5, 4, 8, 6), 0.5, padding=0)
    full = ref.label_map(ones, boxes, (0, 0, 20, 20), 0.5, padding=0)
    assert np.array_equal(win, full[4:10, 5:13])


# ---- the ABI surface, through the built library -------------------------------------------------------------------------------------------
FAKE = 0x10000      # an aligned non-NULL "device pointer": every call below must fail validation before anything dereferences or launches


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


def test_abi_revision_and_registration(lib):
    assert lib.hdy_version() == _lib.ABI_VERSION >= 11
    for name in ('hdy_paste_masks', 'hdy_paste_label_map', 'hdy_label_areas'):
        assert name in _lib.SIGNATURES and lib.hdy_exec_op(name.encode()) >= 0


def test_paste_masks_argument_checks(lib):
    def call(masks=FAKE, R=3, M=28, padding=1, boxes=FAKE, out=FAKE, out_elems=3 * 20 * 30, H=20, W=30):
        return lib.hdy_paste_masks(masks, R, M, padding, boxes, out, out_elems, H, W, None), lib.hdy_last_error()

    for kw in ({'masks': None}, {'boxes': None}, {'out': None}):
        rc, msg = call(**kw)
        assert rc == _lib.EINVAL and b'null' in msg, kw
    for m in (1, 63, 0, -28):
        rc, msg = call(M=m)
        assert rc == _lib.EINVAL and b'M=' in msg and b'[2, 62]' in msg
    for p in (-1, 2):
        rc, msg = call(padding=p)
        assert rc == _lib.EINVAL and b'padding=' in msg
    for n in (3 * 20 * 30 - 1, 3 * 20 * 30 + 1, 0, -1):
        rc, msg = call(out_elems=n)
        assert rc == _lib.EINVAL and b'out_elems' in msg
    assert call(R=-1)[0] == _lib.EINVAL and call(H=0, out_elems=0)[0] == _lib.EINVAL and call(W=-5)[0] == _lib.EINVAL


def test_paste_label_map_argument_checks(lib):
    def call(masks=FAKE, R=3, M=28, padding=1, boxes=FAKE, thr=0.5, x0=0, y0=0, lmap=FAKE, map_elems=20 * 30, h=20, w=30):
        return lib.hdy_paste_label_map(masks, R, M, padding, boxes, thr, x0, y0, lmap, map_elems, h, w, None), lib.hdy_last_error()

    for kw in ({'masks': None}, {'boxes': None}, {'lmap': None}):
        rc, msg = call(**kw)
        assert rc == _lib.EINVAL and b'null' in msg, kw
    assert call(R=0, masks=None, boxes=None, lmap=None)[0] == _lib.EINVAL          # the map is written even without rows
    for m in (1, 63):
        rc, msg = call(M=m)
        assert rc == _lib.EINVAL and b'M=' in msg
    rc, msg = call(padding=2)
    assert rc == _lib.EINVAL and b'padding=2' in msg
    for n in (599, 601, 0):
        rc, msg = call(map_elems=n)
        assert rc == _lib.EINVAL and b'map_elems' in msg
    # 64-bit sizes: a 70 000 x 70 000 window is 4.9e9 entries; the count that 32-bit arithmetic would give is refused
    rc, msg = call(h=70000, w=70000, map_elems=(70000 * 70000) & 0xFFFFFFFF)
    assert rc == _lib.EINVAL and b'map_elems' in msg
    assert call(h=0, map_elems=0)[0] == _lib.EINVAL and call(thr=float('nan'))[0] == _lib.EINVAL


def test_label_areas_argument_checks(lib):
    rc = lib.hdy_label_areas(None, 600, FAKE, 3, None)
    assert rc == _lib.EINVAL and b'null' in lib.hdy_last_error()
    rc = lib.hdy_label_areas(FAKE, 600, None, 3, None)
    assert rc == _lib.EINVAL and b'null' in lib.hdy_last_error()
    assert lib.hdy_label_areas(FAKE, -1, FAKE, 3, None) == _lib.EINVAL and lib.hdy_label_areas(FAKE, 600, FAKE, -3, None) == _lib.EINVAL
    assert lib.hdy_label_areas(None, 0, None, 0, None) == _lib.OK                   # nothing to write: no launch
