"""hdy_label_texture on the device against the numpy restatement of include/hdyolo_texture.h (tests/texture_ref.py), bit for bit, on maps of
at most about 100 x 200 entries; hd_yolo_amd/texture.py's features on the device against their loop restatement; the slide path."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import texture_ref as ref  # noqa: E402
from hd_yolo_amd import _lib, ops  # noqa: E402
from hd_yolo_amd import texture as htexture  # noqa: E402
from test_gpu_mask_rows import mask_model  # noqa: E402,F401  (the module-scoped fixture)
from test_gpu_slide import synth_u8  # noqa: E402

DEV = 'cuda'
OFFS4 = ((0, 1), (-1, 1), (-1, 0), (-1, -1))
H, W, R = 97, 203, 44                 # neither side a multiple of 8 or 64
X0, Y0 = 5, 3                         # where the map's window starts in the image
BIG = 0x7fffffff


def true_extents(lm, R):
    ext = np.tile(np.array([[lm.shape[1], lm.shape[0], -1, -1]], np.int32), (R, 1))
    for r in range(R):
        ii, jj = np.nonzero(lm == r)
        if len(ii):
            ext[r] = (jj.min(), ii.min(), jj.max(), ii.max())
    return ext


def build_case():
    """the map of the module: (lm (H, W) int32, extent (R, 4) int32, rgb window (H, W, 3) uint8, the image with a margin (H + 9, W + 11, 4))"""
    rng = np.random.default_rng(11)
    lm = np.full((H, W), -1, np.int32)
    speck = rng.random((H, W))
    lm[speck < 0.10] = rng.integers(20, R + 3, size=(H, W))[speck < 0.10]            # scattered entries of labels 20 .. R - 1 and of R .. R + 2
    lm[(speck > 0.10) & (speck < 0.13)] = BIG
    lm[(speck > 0.13) & (speck < 0.15)] = -7
    yy, xx = np.mgrid[0:H, 0:W]

    def disc(r, cy, cx, rad):
        lm[(yy - cy) ** 2 + (xx - cx) ** 2 <= rad * rad] = r

    disc(0, 2, 3, 9)                                                      # on the top and left borders
    disc(1, H - 3, W - 4, 10)                                             # on the bottom and right borders
    disc(2, 1, W - 2, 7)                                                  # top right
    # label 3 owns nothing
    lm[50, 100] = 4                                                       # one pixel
    lm[30:33, 40:170] = 5                                                 # 130 columns: three column chunks per row
    lm[20:60, 20:25] = 6                                                  # 40 rows tall
    board = (np.add.outer(np.arange(14), np.arange(22)) & 1).astype(np.int32)
    lm[70:84, 100:122] = 7 + board                                        # labels 7 and 8 interleaved inside one box
    disc(9, 50, 150, 12)
    disc(-1, 52, 149, 5)                                                  # ... with a hole
    disc(10, 10, 60, 6)
    disc(13, 60, 60, 8)
    disc(14, H - 1, 30, 6)                                                # bottom border
    disc(15, 40, 0, 5)                                                    # left border
    disc(16, 80, 190, 11)
    lm[36:39, 26:91] = 17                                                 # 65 columns: one entry into the second chunk
    lm[88:96, 60:68] = 18                                                 # 8 x 8: eight rows per step
    lm[64:67, 84:87] = 19                                                 # 3 x 3: sixteen rows of four columns per step
    ext = true_extents(lm, R)
    ext[10] = (-50, -50, 66, 16)                                          # garbage that still covers the label after the clamp
    ext[11] = (W + 5, H + 5, W + 100, H + 100)                            # beyond the window: empty
    ext[12] = (50, 50, 10, 10)                                            # inverted: empty
    ext[13] = (-BIG - 1, -BIG - 1, BIG, BIG)                              # everything: the window
    ext[20] = (-3, 40, 70, 200)                                           # cuts labels 20's scattered entries: pairs across the box edge count
    ext[21] = (100, -BIG, BIG, 50)
    img = rng.integers(0, 256, size=(H + 9, W + 11, 4)).astype(np.uint8)
    blur = img[Y0:Y0 + H, X0:X0 + W, :3]
    blur[...] = (blur.astype(np.int32) // 3 + (yy[..., None] * 2 + xx[..., None]) // 2) % 256          # neighbouring pixels of nearby levels
    return lm, ext, np.ascontiguousarray(img[Y0:Y0 + H, X0:X0 + W, :3]), img


@pytest.fixture(scope='module')
def case():
    lm, ext, rgb, img = build_case()
    return dict(lm=lm, ext=ext, rgb=rgb, img=img, lm_d=torch.from_numpy(lm).to(DEV), ext_d=torch.from_numpy(ext).to(DEV), want={})


def lut_for(levels, seed=3):
    """a table whose sums fall below zero and above the top level for part of the colours (both clamps), most of them in between"""
    rng = np.random.default_rng(seed)
    top = (1 << 16) * levels
    return rng.integers(-top // 8, top // 2, size=(3, 256)).astype(np.int32)


def image_view(img, pixel_stride):
    """the image on the device as a view with a padded row stride, 3 or 4 bytes per pixel"""
    hh, ww = img.shape[:2]
    wide = torch.full((hh, ww + 5, pixel_stride), 0x55, dtype=torch.uint8, device=DEV)
    wide[:, :ww] = torch.from_numpy(np.ascontiguousarray(img[:, :, :pixel_stride])).to(DEV)
    return wide[:, :ww]


def run_raw(lm_d, R, ext_d, image, lut_d, levels, offsets, window, row0, rows):
    """hdy_label_texture through _ext.call into outputs pre-filled with 0x7f bytes"""
    from hd_yolo_amd import _ext
    D = len(offsets)
    h, w = lm_d.shape
    ip, pitch, pb, IH, IW = ops.slide_u8(image)
    outs = [torch.full(s, 0x7f7f7f7f, dtype=torch.int32, device=DEV) for s in ((rows, levels), (rows, D, levels, levels), (rows,))]
    host = (ctypes.c_int * (2 * D))(*(v for o in offsets for v in o))
    _ext.call('hdy_label_texture', lm_d.data_ptr(), lm_d.numel(), h, w, ip, (IH - 1) * pitch + IW * pb, pitch, pb, window[0], window[1],
              ext_d.data_ptr(), ext_d.numel(), R, lut_d.data_ptr(), 768, levels, host, 2 * D, D, row0, rows,
              *(v for o in outs for v in (o.data_ptr(), o.numel())), ops.stream_ptr())
    return [o.cpu().numpy() for o in outs]


def expect(case, lut, levels, offsets):
    key = (lut.tobytes(), levels, tuple(offsets))
    if key not in case['want']:
        case['want'][key] = ref.texture_vec(case['lm'], case['rgb'], case['ext'], lut, levels, offsets)
    return case['want'][key]


def assert_same(got, want, what=''):
    for name, g, w in zip(('hist', 'glcm', 'flags'), got, want):
        assert g.dtype == np.int32 and g.shape == w.shape and np.array_equal(g, w), (what, name, np.argwhere(g != w)[:5].tolist())


@pytest.mark.parametrize('levels, offsets, pixel_stride', [
    (16, OFFS4, 3),
    (8, ((0, 1), (0, -1)), 4),
    (32, ((4, -4), (-3, 2), (1, 0), (0, 4)), 4),
    (32, ((-4, 0),), 3),
    (16, ((1, 1), (2, -1), (-4, 4)), 4),
    (8, OFFS4, 3)])
def test_counts_equal_the_restatement_bit_for_bit(case, levels, offsets, pixel_stride):
    lut = lut_for(levels)
    want = expect(case, lut, levels, offsets)
    hist, glcm, flags = want
    lev = ref.levels_of(case['rgb'], lut, levels)
    assert (lev == 0).any() and (lev == levels - 1).any() and len(np.unique(lev)) == levels                # both clamps and everything between
    t = lut.astype(np.int64)[0][case['rgb'][..., 0]] + lut.astype(np.int64)[1][case['rgb'][..., 1]] + lut.astype(np.int64)[2][case['rgb'][..., 2]]
    assert (t < 0).any() and ((t >> 16) >= levels).any()
    assert flags.tolist()[:14] == [0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 1, 1, 0] and hist[4].sum() == 1 and not glcm[4].any()
    assert hist[5].sum() == 3 * 130 and hist[6].sum() == 40 * 5 and hist[7].sum() == hist[8].sum() == 7 * 22 and hist[17].sum() == 3 * 65
    image = image_view(case['img'], pixel_stride)
    assert image.stride(0) == (W + 11 + 5) * pixel_stride
    lut_d = torch.from_numpy(lut).to(DEV)
    _lib.dispatch_log(reset=True)
    got = run_raw(case['lm_d'], R, case['ext_d'], image, lut_d, levels, offsets, (X0, Y0), 0, R)
    assert _lib.dispatch_log(reset=True) == ['label_texture']
    assert_same(got, want, 'whole call')
    # the same call twice gives equal bits
    again = run_raw(case['lm_d'], R, case['ext_d'], image, lut_d, levels, offsets, (X0, Y0), 0, R)
    assert_same(again, got, 'repeat')
    # rows sub-ranges whose concatenation is the whole call
    parts = [run_raw(case['lm_d'], R, case['ext_d'], image, lut_d, levels, offsets, (X0, Y0), a, n) for a, n in ((0, 1), (1, 6), (7, 30), (37, R - 37))]
    assert_same([np.concatenate([p[k] for p in parts]) for k in range(3)], want, 'row ranges')
    # ops.label_texture: the same bits, tensors of the stated shapes on the device
    h2, g2, f2 = ops.label_texture(case['lm_d'], R, case['ext_d'], image, lut_d, levels, offsets, window=(X0, Y0), rows=(7, 30))
    assert h2.shape == (30, levels) and g2.shape == (30, len(offsets), levels, levels) and f2.shape == (30,) and g2.device.type == 'cuda'
    assert_same([t.cpu().numpy() for t in (h2, g2, f2)], [v[7:37] for v in want], 'ops rows')


def test_checkerboard_labels_and_the_hole_against_the_loop(case):
    """the entry-by-entry restatement on the labels where the other build could share a mistake: interleaved labels, the hole, the borders"""
    lut = lut_for(16)
    want = expect(case, lut, 16, OFFS4)
    for r in (0, 1, 7, 8, 9, 14, 20):
        loop = ref.texture_loop(case['lm'], case['rgb'], case['ext'], lut, 16, OFFS4, row0=r, rows=1)
        for a, b in zip(loop, want):
            assert np.array_equal(a[0], b[r]), r
    glcm = want[1]
    assert not glcm[7, 0].any() and not glcm[7, 2].any() and glcm[7, 1].any() and glcm[7, 3].any()      # a checkerboard has diagonal partners only


def test_any_table_content_wraps_modulo_2_to_32(case):
    lut = np.random.default_rng(21).integers(-BIG - 1, BIG, size=(3, 256), endpoint=True).astype(np.int32)
    t = lut.astype(np.int64)[0][case['rgb'][..., 0]] + lut.astype(np.int64)[1][case['rgb'][..., 1]] + lut.astype(np.int64)[2][case['rgb'][..., 2]]
    assert (t > BIG).any() and (t < -BIG - 1).any()                       # sums that leave 32 bits on both sides
    want = expect(case, lut, 16, ((0, 1), (1, 0)))
    got = run_raw(case['lm_d'], R, case['ext_d'], image_view(case['img'], 3), torch.from_numpy(lut).to(DEV), 16, ((0, 1), (1, 0)), (X0, Y0), 0, R)
    assert_same(got, want, 'wrapping table')


def test_a_box_side_of_1025_is_skipped_and_1024_is_not():
    rng = np.random.default_rng(5)
    for shape, line0, line1, ext in (((3, 1030), (1, slice(2, 1027)), (2, slice(3, 1027)), [[2, 1, 1026, 1], [3, 2, 1026, 2]]),
                                     ((1030, 2), (slice(0, 1025), 0), (slice(6, 1030), 1), [[0, 0, 0, 1024], [1, 6, 1, 1029]])):
        lm = np.full(shape, -1, np.int32)
        lm[line0], lm[line1] = 0, 1
        rgb = rng.integers(0, 256, size=shape + (3,)).astype(np.uint8)
        ext = np.array(ext, np.int32)
        lut = lut_for(16, seed=9)
        want = ref.texture_vec(lm, rgb, ext, lut, 16, OFFS4)
        assert want[2].tolist() == [2, 0] and not want[0][0].any() and not want[1][0].any() and want[0][1].sum() == 1024 and want[1][1].sum() == 2 * 1023
        got = run_raw(torch.from_numpy(lm).to(DEV), 2, torch.from_numpy(ext).to(DEV), torch.from_numpy(rgb).to(DEV), torch.from_numpy(lut).to(DEV),
                      16, OFFS4, (0, 0), 0, 2)
        assert_same(got, want, shape)


def test_ops_refuse_what_the_kernel_cannot_take(case):
    lm, ext = case['lm_d'], case['ext_d']
    image = image_view(case['img'], 3)
    lut = torch.from_numpy(lut_for(16)).to(DEV)
    ok = dict(label_map=lm, R=R, extent=ext, image=image, lut=lut, levels=16, window=(X0, Y0))
    for kw, word in ((dict(lut=lut.cpu()), 'on CPU'), (dict(lut=lut.long()), 'lut must be an int32 (3, 256)'), (dict(lut=lut[:, :255]), 'lut must be'),
                     (dict(extent=ext[:-1]), 'extent must be'), (dict(extent=ext.long()), 'extent must be'), (dict(label_map=lm.long()), 'int32'),
                     (dict(image=None), 'needs the 8-bit image'), (dict(image=image.float()), 'uint8'), (dict(window=(X0 + 7, Y0)), 'leaves the'),
                     (dict(window=(-1, 0)), 'leaves the'), (dict(levels=12), 'levels=12'), (dict(offsets=()), '0 offsets'),
                     (dict(offsets=((0, 1),) * 5), '5 offsets'), (dict(rows=(40, 5)), 'rows=(40, 5)'), (dict(rows=(-1, 2)), 'rows=(-1, 2)'),
                     (dict(offsets=((0, 5),)), 'reaches beyond 4'), (dict(offsets=((0, 0),)), '(0, 0)')):
        with pytest.raises(_lib.HdyError) as e:
            ops.label_texture(**dict(ok, **kw))
        assert word in str(e.value), (kw, str(e.value))
    _lib.dispatch_log(reset=True)
    h0, g0, f0 = ops.label_texture(**dict(ok, rows=(R, 0)))
    assert h0.shape == (0, 16) and g0.shape == (0, 4, 16, 16) and f0.shape == (0,) and _lib.dispatch_log() == []


def test_features_on_the_device_equal_the_loop_restatement(case):
    """float64 sums of at most 1 024 terms in different orders: relative error of order 1 024 * 2^-53, far inside rtol 1e-9; imc2 through
    its square, because the root of a difference near zero turns 1e-13 into 1e-6"""
    lut = lut_for(16)
    hist, glcm, flags = expect(case, lut, 16, OFFS4)
    got = htexture.haralick(torch.from_numpy(glcm).to(DEV))
    assert got.dtype == torch.float64 and got.shape == (R, 4, 13) and got.device.type == 'cuda'
    got = got.cpu().numpy()
    want = np.array([[ref.haralick_loop(glcm[q, d]) for d in range(4)] for q in range(R)])
    got[..., 12], want[..., 12] = got[..., 12] ** 2, want[..., 12] ** 2
    assert np.isnan(want[3]).all() and np.isnan(want[4]).all() and np.isfinite(want[[0, 1, 5, 6, 9, 16]]).all()
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-12, equal_nan=True)
    stats = htexture.intensity(torch.from_numpy(hist).to(DEV), 16)
    got_i = np.stack([stats[k].cpu().numpy() for k in htexture.INTENSITY], 1)
    np.testing.assert_allclose(got_i, np.array([ref.intensity_loop(hv) for hv in hist]), rtol=1e-9, atol=1e-12, equal_nan=True)
    # texture_table in chunks that do not divide R: the same columns as one chunk, bit for bit, and the counts' flags
    image = image_view(case['img'], 4)
    one = htexture.texture_table(case['lm_d'], R, case['ext_d'], image, window=(X0, Y0), stain='eosin', levels=16)
    parts = htexture.texture_table(case['lm_d'], R, case['ext_d'], image, window=(X0, Y0), stain='eosin', levels=16, chunk=13)
    assert list(one) == list(parts) and len(one) == 8 + 26 + 1
    for k in one:
        assert one[k].dtype == torch.float64 and one[k].shape == (R,), k
        assert torch.equal(torch.nan_to_num(one[k], nan=-1.0), torch.nan_to_num(parts[k], nan=-1.0)), k
    assert one['tex_flags'].tolist() == flags.tolist()
    e_lut = htexture.stain_lut('eosin', 16).numpy()
    e_hist, e_glcm, _ = ref.texture_vec(case['lm'], case['rgb'], case['ext'], e_lut, 16, OFFS4)
    np.testing.assert_allclose(one['tex_level_mean'].cpu().numpy(), [ref.intensity_loop(hv)[0] for hv in e_hist], rtol=1e-9, atol=1e-12, equal_nan=True)
    contrast = np.array([[ref.haralick_loop(e_glcm[q, d])[1] for d in range(4)] for q in range(R)])
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                                   # a row of NaN has no mean: NaN is what the table holds there
        want_c = np.nanmean(contrast, 1)
    np.testing.assert_allclose(one['tex_contrast_mean'].cpu().numpy(), want_c, rtol=1e-9, atol=1e-12, equal_nan=True)


FILLED = 0.2          # a paste threshold below every value of the synthetic mask head (see slide_runs)


@pytest.fixture(scope='module')
def slide_runs(mask_model):
    """One 512 x 512 synthetic 8-bit slide through the synthetic mask model, once; per paste threshold its label map, its nucleus table and
    its texture columns: threshold -> (slide, result, columns, dispatch log of slide_nucleus_texture).

    The synthetic mask head has random weights: its 28 x 28 masks are noise between 0.35 and 0.53 (1st and 99th percentile, median 0.44).
    At the default threshold 0.5 one entry in a hundred of a box is pasted, so a label is a handful of isolated entries (`#.....#`): no
    entry has a partner at distance 1 and, as the header's convention has it, the label has a histogram and no co-occurrence.  That is
    worth testing (exactly the unpaired labels are NaN) but it is not what a mask is.  At FILLED = 0.2, below every value, a detection owns
    its box except what higher-scoring boxes own: labels are regions whose entries touch, as a nucleus's do, and that is the map on which
    "finite wherever the area is at least 2" is asked."""
    import evaluation
    _, dep = mask_model
    slide = synth_u8(512, 7).to(DEV)
    det = evaluation.inference_on_slide(dep, slide, tile=256, overlap=32, batch_size=8, compute_masks=True)['det']
    assert len(det['boxes']) > 0, 'the synthetic mask model found nothing on the slide: the test needs detections'
    runs = {}
    for threshold in (0.5, FILLED):
        res = dict(det)
        res['label_map'], _ = evaluation.slide_label_map(res, (512, 512), threshold=threshold)
        res['nuclei'] = evaluation.slide_nucleus_table(res, slide=slide)
        _lib.dispatch_log(reset=True)
        cols = evaluation.slide_nucleus_texture(res, slide)
        runs[threshold] = (slide, res, cols, _lib.dispatch_log(reset=True))
    return runs


@pytest.mark.parametrize('threshold', [0.5, FILLED])
def test_slide_nucleus_texture(slide_runs, threshold):
    import evaluation
    slide, res, cols, log = slide_runs[threshold]
    n = len(res['boxes'])
    assert log == ['label_texture']
    assert len(cols) == 35 and all(v.shape == (n,) and v.dtype == torch.float64 and v.device.type == 'cuda' for v in cols.values())     # one row per detection
    area = res['nuclei']['area']
    assert bool((cols['tex_flags'][area == 0] == 1).all()) and bool((cols['tex_flags'][area > 0] == 0).all())
    for k in htexture.INTENSITY:
        assert bool(torch.isfinite(cols[f'tex_{k}'][area >= 1]).all()), k
    sums, extent = ops.label_measure(res['label_map'], n)
    direct = htexture.texture_table(res['label_map'], n, extent, slide)
    for k, v in cols.items():
        assert torch.equal(torch.nan_to_num(v, nan=-1.0), torch.nan_to_num(direct[k], nan=-1.0)), k                   # bit-equal
    # the counts under the columns, against the restatement on the returned map (two ranges of labels: the restatement takes a map pass each)
    lut = htexture.stain_lut('hematoxylin', 16)
    hist, glcm, flags = ops.label_texture(res['label_map'], n, extent, slide, lut.to(DEV))
    assert torch.equal(hist.sum(1).long(), area)
    host = [t.cpu().numpy() for t in (hist, glcm, flags)]
    for row0, rows in ((0, min(n, 120)), (n // 2, min(n - n // 2, 120))):
        want = ref.texture_vec(res['label_map'].cpu().numpy(), slide.cpu().numpy(), extent.cpu().numpy(), lut.numpy(), 16, OFFS4, row0, rows)
        assert_same([t[row0:row0 + rows] for t in host], want, ('slide', row0))
    # a label has finite features exactly where one of its entries has a partner in one of the four directions
    paired = glcm.sum((1, 2, 3)) > 0
    assert int(paired.sum()) > 0
    if threshold == 0.5:
        assert int(((area >= 2) & ~paired).sum()) > 0                     # the isolated entries of the docstring above
    for name in htexture.FEATURES:
        for kind in ('mean', 'range'):
            assert torch.equal(torch.isfinite(cols[f'tex_{name}_{kind}']), paired), (name, kind)
    with pytest.raises(ValueError, match="needs 'label_map' and 'nuclei'"):
        evaluation.slide_nucleus_texture({'boxes': res['boxes']}, slide)


def test_slide_columns_are_finite_where_the_area_is_at_least_2(slide_runs):
    """every column finite wherever area >= 2 and the flag is 0, on the map whose labels are regions (slide_runs says why not on the other)"""
    slide, res, cols, _ = slide_runs[FILLED]
    area = res['nuclei']['area']
    measured = (area >= 2) & (cols['tex_flags'] == 0)
    assert int(measured.sum()) >= 100                                     # most detections, not a remnant
    nan = {k: int((~torch.isfinite(v[measured])).sum()) for k, v in cols.items()}
    print(f'{len(area)} detections, {int(measured.sum())} with area >= 2 and flag 0; columns with non-finite rows among them: '
          f'{ {k: c for k, c in nan.items() if c} }')
    for k, v in cols.items():
        assert bool(torch.isfinite(v[measured]).all()), k
