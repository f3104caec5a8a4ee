"""Host-side checks of the 8-bit whole-slide path (no GPU): the three entry points of csrc/slide.hip reject bad arguments with a status and a
message before any launch (tests/test_abi.py's FAKE pointer style), the host side of the tile table follows a numpy restatement kept here,
and evaluation.inference_on_slide refuses slides it cannot take with a clear error."""
import os

import numpy as np
import pytest
import torch

from hd_yolo_amd import _lib, build

FAKE = 0x10000      # a 16-byte aligned non-NULL "device pointer": every call below must fail validation before anything dereferences or launches


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


def tiles(lib, pixel_bytes=3, pitch=None, H=1000, W=1000, n=10, first=0, count=4, out_elems=None, th=128, tw=128, pad=2, ldd=0, slide=FAKE,
          origins=FAKE, out=FAKE, dtype=_lib.BF16):
    pitch = W * pixel_bytes if pitch is None else pitch
    if out_elems is None:
        out_elems = count * (th + 2 * pad) * (tw + 2 * pad) * 4 if ldd == 0 else count * th * tw * ldd
    return lib.hdy_slide_tiles_u8(slide, pitch, pixel_bytes, H, W, origins, n, first, count, out, out_elems, th, tw, pad, ldd, dtype, None)


def test_tile_gather_rejects_bad_arguments_before_any_launch(lib):
    err = lib.hdy_last_error
    for pb in (0, 1, 2, 5, 8):
        assert tiles(lib, pixel_bytes=pb, pitch=4000) == _lib.EINVAL and b'pixel_bytes' in err()
    assert tiles(lib, pixel_bytes=3, pitch=2999) == _lib.EINVAL and b'pitch' in err()
    assert tiles(lib, pixel_bytes=4, pitch=3999) == _lib.EINVAL and b'pitch' in err()
    assert tiles(lib, n=10, first=7, count=4) == _lib.EINVAL and b'origin table' in err()
    assert tiles(lib, n=10, first=-1, count=4) == _lib.EINVAL
    assert tiles(lib, n=10, first=0, count=0) == _lib.EINVAL
    assert tiles(lib, n=10, first=(1 << 31) - 2, count=4) == _lib.EINVAL        # first + count must not wrap
    want = 4 * 132 * 132 * 4
    for bad in (want - 1, want + 1, 4 * 128 * 128 * 4, 0):
        assert tiles(lib, out_elems=bad) == _lib.EINVAL and b'out holds' in err()
    assert tiles(lib, ldd=8, pad=0, out_elems=4 * 128 * 128 * 8 - 8) == _lib.EINVAL and b'out holds' in err()
    assert tiles(lib, ldd=8, pad=2, out_elems=4 * 128 * 128 * 8) == _lib.EINVAL      # a pitched NHWC input has no frame
    assert tiles(lib, ldd=2, pad=0, out_elems=4 * 128 * 128 * 2) == _lib.EINVAL
    assert tiles(lib, slide=None) == _lib.EINVAL and b'null' in err()
    assert tiles(lib, origins=None) == _lib.EINVAL and tiles(lib, out=None) == _lib.EINVAL
    assert tiles(lib, out=FAKE + 8) == _lib.EINVAL and b'aligned' in err()
    assert tiles(lib, dtype=7) == _lib.EINVAL
    assert tiles(lib, H=0) == _lib.EINVAL and tiles(lib, th=0) == _lib.EINVAL and tiles(lib, pad=-1) == _lib.EINVAL


def append(lib, B=4, in_rows=1200, n=10, first=0, capacity=3000, boxes=FAKE, cursor=FAKE):
    return lib.hdy_slide_append(boxes, FAKE, FAKE, FAKE, B, in_rows, FAKE, n, first, FAKE, FAKE, FAKE, capacity, cursor, None)


def test_append_rejects_bad_arguments_before_any_launch(lib):
    err = lib.hdy_last_error
    assert append(lib, capacity=0) == _lib.EINVAL and b'capacity' in err()
    assert append(lib, capacity=-5) == _lib.EINVAL
    assert append(lib, n=10, first=8, B=4) == _lib.EINVAL and b'origin table' in err()
    assert append(lib, B=0) == _lib.EINVAL and append(lib, B=1025) == _lib.EINVAL and b'batch' in err()
    assert append(lib, in_rows=0) == _lib.EINVAL
    assert append(lib, boxes=None) == _lib.EINVAL and b'null' in err()
    assert append(lib, cursor=None) == _lib.EINVAL
    assert append(lib, boxes=FAKE + 4) == _lib.EINVAL and b'aligned' in err()


def test_tissue_rejects_bad_arguments_before_any_launch(lib):
    err = lib.hdy_last_error

    def tissue(pixel_bytes=3, pitch=3000, H=1000, W=1000, n=10, n_counts=10, th=128, tw=128, background=220, slide=FAKE, counts=FAKE):
        return lib.hdy_slide_tissue_u8(slide, pitch, pixel_bytes, H, W, FAKE, n, th, tw, background, counts, n_counts, None)

    assert tissue(pixel_bytes=2) == _lib.EINVAL and b'pixel_bytes' in err()
    assert tissue(pitch=2999) == _lib.EINVAL and b'pitch' in err()
    assert tissue(pixel_bytes=4, pitch=3999) == _lib.EINVAL
    assert tissue(n_counts=9) == _lib.EINVAL and b'counts' in err()
    assert tissue(n=0, n_counts=0) == _lib.EINVAL
    assert tissue(background=-1) == _lib.EINVAL and tissue(background=300) == _lib.EINVAL
    assert tissue(slide=None) == _lib.EINVAL and tissue(counts=None) == _lib.EINVAL
    assert tissue(tw=0) == _lib.EINVAL


def test_the_three_entry_points_can_be_listed_for_the_executor(lib):
    for name in (b'hdy_slide_tiles_u8', b'hdy_slide_append', b'hdy_slide_tissue_u8'):
        assert lib.hdy_exec_op(name) >= 0


# ---- the tile table: numpy restatement of slide_rois and of the tissue rule ------------------------------------------------------------------
def starts_ref(n, tile, overlap):
    if n <= tile:
        return np.array([0])
    s = np.arange(0, n - tile, tile - overlap)
    return np.unique(np.concatenate([s, [n - tile]]))


def table_ref(H, W, tile, overlap):
    ys, xs = starts_ref(H, tile, overlap), starts_ref(W, tile, overlap)
    return np.stack([np.tile(xs, len(ys)), np.repeat(ys, len(xs))], 1).astype(np.int32)


def tissue_ref(slide, table, tile, background):
    """pixels of each window (clipped to the slide) with min(R, G, B) < background"""
    t = slide[:, :, :3].min(axis=2) < background
    return np.array([t[y0:y0 + tile, x0:x0 + tile].sum() for x0, y0 in table], dtype=np.int64)


def keep_ref(counts, min_tissue, tile):
    return counts >= min_tissue * tile * tile


@pytest.mark.parametrize('H,W,tile,overlap', [(256, 256, 128, 0), (448, 448, 128, 64), (200, 300, 128, 32), (100, 100, 128, 0), (300, 128, 128, 32),
                                              (1000, 777, 160, 16)])
def test_tile_table_follows_slide_rois(H, W, tile, overlap):
    import evaluation
    got = evaluation.slide_tile_table(H, W, tile, overlap)
    assert got.dtype == np.int32 and got.shape[1] == 2
    assert got.tolist() == [list(r) for r in evaluation.slide_rois(H, W, tile, overlap)]
    assert np.array_equal(got, table_ref(H, W, tile, overlap))
    assert (got[:, 0] + min(tile, W) <= W).all() and (got[:, 1] + min(tile, H) <= H).all() and (got >= 0).all()


def test_tile_table_drops_rows_under_min_tissue():
    import evaluation
    rng = np.random.default_rng(3)
    H, W, tile, overlap = 300, 400, 128, 32
    slide = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    slide[:, W // 2:] = 255                                              # the right half is glass
    slide[:40, :60] = 230                                                # light, above the default background of 220
    table = table_ref(H, W, tile, overlap)
    for background, min_tissue in ((220, 0.05), (220, 0.5), (255, 0.3), (0, 0.01), (220, 0.0)):
        counts = tissue_ref(slide, table, tile, background)
        got = evaluation.slide_tile_table(H, W, tile, overlap, counts, min_tissue)
        want = table[keep_ref(counts, min_tissue, tile)] if min_tissue > 0 else table
        assert np.array_equal(got, want), (background, min_tissue)
    counts = tissue_ref(slide, table, tile, 220)
    kept = evaluation.slide_tile_table(H, W, tile, overlap, counts, 0.05)
    assert 0 < len(kept) < len(table)
    # a tile straddling the middle stays, the all-glass tiles of the right edge go
    assert any(x0 < W // 2 < x0 + tile for x0, _ in kept) and not any(x0 >= W // 2 for x0, _ in kept)
    # the boundary: count == min_tissue * tile * tile stays
    assert len(evaluation.slide_tile_table(128, 128, 128, 0, [8192], 0.5)) == 1 and len(evaluation.slide_tile_table(128, 128, 128, 0, [8191], 0.5)) == 0
    assert evaluation.slide_tile_table(128, 128, 128, 0, [0], 0.5).shape == (0, 2)


def test_inference_on_slide_refuses_what_it_cannot_take():
    import evaluation
    model = object()                                                     # never reached: the slide is checked first
    with pytest.raises(ValueError, match='must be on the GPU'):
        evaluation.inference_on_slide(model, torch.zeros((3, 64, 64)))
    with pytest.raises(ValueError, match='must be on the GPU'):
        evaluation.inference_on_slide(model, torch.zeros((64, 64, 3), dtype=torch.uint8))
    with pytest.raises(TypeError, match='torch tensor'):
        evaluation.inference_on_slide(model, np.zeros((64, 64, 3), dtype=np.uint8))


def test_eight_bit_slide_layouts_are_checked_by_one_rule():
    """the layout rule itself (shape, strides), on CPU tensors standing in for device ones: the planar (3, H, W) uint8 slide, a channel-strided
    view, a transposed view and a negative / short row stride are refused; RGB, RGBA and a crop of a larger slide pass"""
    import evaluation

    class _Cuda(torch.Tensor):
        """a CPU tensor that says it is on the GPU: the rule reads dtype, shape and strides only"""

        @property
        def is_cuda(self):
            return True

    def check(t):
        return evaluation._check_slide(t.as_subclass(_Cuda))

    big = torch.zeros((200, 300, 4), dtype=torch.uint8)
    assert check(torch.zeros((64, 80, 3), dtype=torch.uint8)) is True
    assert check(big) is True
    assert check(big[10:150, 7:206]) is True                            # a crop: row pitch larger than the row
    assert check(torch.zeros((3, 8, 8))) is False                        # the float slide
    for bad in (torch.zeros((3, 64, 80), dtype=torch.uint8), big[:, :, :3], big.transpose(0, 1), big[:, ::2], torch.zeros((64, 80), dtype=torch.uint8),
                torch.zeros((64, 80, 1), dtype=torch.uint8), torch.zeros((0, 80, 3), dtype=torch.uint8)):
        with pytest.raises(ValueError, match='8-bit slide must be'):
            check(bad)
    with pytest.raises(ValueError, match='float'):
        check(torch.zeros((3, 8, 8), dtype=torch.int32))
    with pytest.raises(ValueError, match='float'):
        check(torch.zeros((8, 8)))
