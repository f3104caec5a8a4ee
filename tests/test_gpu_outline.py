"""Outlines and hulls on the MI355X (csrc/outline.hip: hdy_label_outline_count, hdy_label_outline_write, hdy_label_hull), through the entry
points with poisoned buffers of the test's own, through ops.label_outline / ops.label_hull, hd_yolo_amd/outline.py and
evaluation.inference_on_slide(..., outlines=True).  offsets, verts, counts and hull_i are compared bit for bit with the restatement
(tests/outline_ref.py), which tests/test_outline_host.py ties to answers derived by hand; hull_f within 1e-9 relative.

That bound is derived, not measured: the perimeter is a sum of at most ~4100 square roots of exact integers, each within 1 ulp, the minimum
Feret diameter takes two roundings, so the error stays near 1e-12 and 1e-9 leaves about three orders of margin; ties between hull edges change
which edge attains the minimum, never its value."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import measure_ref as mref  # noqa: E402
import outline_ref as ref  # noqa: E402
from hd_yolo_amd import _ext, _lib, ops  # noqa: E402
from hd_yolo_amd import outline as houtline  # noqa: E402
from test_gpu_mask_rows import mask_model  # noqa: E402,F401  (the module-scoped fixture)
from test_gpu_slide import synth_u8  # noqa: E402

DEV = torch.device('cuda', 0)
POISON = -0x5A5A5A5B
TAIL = 8             # rows of verts behind `total` that the writing pass must leave alone
RTOL = 1e-9


def poisoned(shape, dtype):
    t = torch.empty(shape, dtype=dtype, device=DEV)
    return t.fill_(float('nan')) if dtype.is_floating_point else t.fill_(POISON)


def write_pass(lm, R, extent, offsets):
    """hdy_label_outline_write into a poisoned buffer with TAIL rows behind the last offset -> (verts with the tail, status)"""
    total = max(int(offsets[-1]), 0)
    verts = poisoned((total + TAIL, 2), torch.int32)
    status = poisoned((1,), torch.int32)
    _ext.call('hdy_label_outline_write', lm.data_ptr(), lm.numel(), lm.shape[0], lm.shape[1], extent.data_ptr(), extent.numel(), R,
              offsets.data_ptr(), offsets.numel(), verts.data_ptr(), 2 * total, status.data_ptr(), ops.stream_ptr())
    return verts, int(status)


def device_run(lm, R, extent):
    """the three passes on device tensors with poisoned outputs -> numpy (offsets, verts, counts, hull_i, hull_f)"""
    head = (lm.data_ptr(), lm.numel(), lm.shape[0], lm.shape[1], extent.data_ptr(), extent.numel(), R)
    counts = poisoned((R, 4), torch.int64)
    _ext.call('hdy_label_outline_count', *head, counts.data_ptr(), counts.numel(), ops.stream_ptr())
    offsets = torch.zeros((R + 1,), dtype=torch.int64, device=DEV)
    offsets[1:] = torch.cumsum(counts[:, 0], 0)
    verts, status = write_pass(lm, R, extent, offsets)
    total = int(offsets[-1])
    assert status == 0
    assert bool((verts[total:] == POISON).all()), 'rows of verts past total were written'
    hull_i, hull_f = poisoned((R, 4), torch.int64), poisoned((R, 2), torch.float64)
    _ext.call('hdy_label_hull', *head, hull_i.data_ptr(), hull_i.numel(), hull_f.data_ptr(), hull_f.numel(), ops.stream_ptr())
    return tuple(t.cpu().numpy() for t in (offsets, verts[:total], counts, hull_i, hull_f))


def assert_equal_to(got, want):
    for name, g, w in zip(('offsets', 'verts', 'counts', 'hull_i'), got, want):
        assert g.shape == w.shape and np.array_equal(g, w), (name, np.argwhere(g != w)[:6] if g.shape == w.shape else (g.shape, w.shape))
    np.testing.assert_allclose(got[4], want[4], rtol=RTOL, atol=0)


def check(lm, R, extent=None, want=None):
    """both runs of the three passes against the restatement; extent: None = the map's own (measure_ref)"""
    if extent is None:
        extent = mref.measure(lm, R)[1]
    lm_d, ext_d = torch.from_numpy(lm).to(DEV), torch.from_numpy(np.ascontiguousarray(extent, dtype=np.int32)).to(DEV)
    got = device_run(lm_d, R, ext_d)
    again = device_run(lm_d, R, ext_d)
    for g, a in zip(got, again):
        assert np.array_equal(g, a)                                                       # hull_f too: a fixed order of sums
    if want is None:
        want = ref.outlines(lm, R, extent) + ref.hulls(lm, R, extent)
    assert_equal_to(got, want)
    return got


@pytest.mark.parametrize('h,w', [(1, 1), (1, 63), (3, 65), (5, 130), (33, 64), (70, 150)])
def test_small_windows(h, w):
    """boxes narrower and wider than a wave's 64 columns, heights that are no multiple of the four rows in flight, labels on every border;
    stripes: one label over whole rows, in several fragments once h > 2 R; one label everywhere"""
    rng = np.random.default_rng(h * 1000 + w)
    R = 7
    check(mref.random_map(rng, h, w, R), R)
    stripes = np.repeat((np.arange(h, dtype=np.int32) // 2 % R)[:, None], w, 1)
    got = check(stripes, R)
    assert got[2][0].tolist() == [4, 2 * w * min(h, 2), 2 * (w + min(h, 2)), 0]
    got = check(np.zeros((h, w), dtype=np.int32), 1)
    assert got[1].tolist() == [[0, 0], [w, 0], [w, h], [0, h]] and got[3][0].tolist() == [4, 2 * h * w, h * h + w * w, 0]


@pytest.mark.parametrize('name', list(ref.HAND))
def test_hand_shapes(name):
    lm, verts, area2, L, n, simple, hi, hf = ref.HAND[name]
    lm = np.pad(lm, ((2, 1), (3, 2)), constant_values=-1)
    got = check(lm, 1)
    assert (got[1] - np.array([3, 2])).tolist() == [list(p) for p in verts] and got[2][0].tolist() == [len(verts), area2, L, 0]
    assert got[3][0].tolist() == list(hi) + [0]
    np.testing.assert_allclose(got[4][0], hf, rtol=RTOL)


@pytest.mark.parametrize('R', [4096, 100])
def test_every_entry_its_own_label(R):
    """64 x 64 with 4096 different values: every outline a unit square; with R = 100 most values are background"""
    lm = np.random.default_rng(2).permutation(4096).astype(np.int32).reshape(64, 64)
    ii, jj = np.divmod(np.argsort(lm.ravel())[:R], 64)
    square = np.stack([np.stack([jj + a, ii + b], 1) for a, b in ((0, 0), (1, 0), (1, 1), (0, 1))], 1).reshape(-1, 2).astype(np.int32)
    want = (np.arange(R + 1, dtype=np.int64) * 4, square, np.tile(np.array([4, 2, 4, 0], dtype=np.int64), (R, 1)),
            np.tile(np.array([4, 2, 2, 0], dtype=np.int64), (R, 1)), np.tile(np.array([4.0, 1.0]), (R, 1)))
    check(lm, R, want=want)
    if R == 100:
        check(lm, R)                                                                      # and the restatement says the same


def test_non_labels_are_background_and_safe():
    R = 5
    lm = np.array([[-1, -7, 0x7fffffff, R, 0, 0, -(2 ** 31), R + 1], [4, 4, 4, R, 0x7fffffff, 2, 2, -1]], dtype=np.int32)
    got = check(lm, R)
    assert got[2][:, 0].tolist() == [4, 0, 4, 0, 4] and got[2][:, 3].tolist() == [0, 1, 0, 1, 0]
    big = np.random.default_rng(3).choice(np.array([-1, -7, 0x7fffffff, R], dtype=np.int64), size=(70, 150)).astype(np.int32)
    got = check(big, R)
    assert len(got[1]) == 0 and (got[2][:, 3] == 1).all() and (got[3][:, 3] == 1).all()


def test_one_pixel_beside_a_comb_in_one_wave():
    """lanes 0 and 1 of one wave: a unit square and an outline of tens of thousands of cracks (divergence), whose walk ends far below its cap"""
    lm = np.full((204, 206), -1, dtype=np.int32)
    lm[1, 1] = 0
    lm[2, 4:204] = 1
    lm[2:202, 4:204:2] = 1                                                                # a spine and 100 teeth of 199 pixels
    got = check(lm, 2)
    n = 200 + 100 * 199
    assert got[2][0].tolist() == [4, 2, 4, 0] and got[2][1, 1:].tolist() == [2 * n, 2 * n + 2, 0]      # a tree of pixels: 4 n - 2 (n - 1) cracks
    assert got[2][1, 0] > 400 and got[3][1, 0] == 5


def test_a_label_wider_than_the_side_bound_is_skipped():
    lm = np.full((6, 1100), -1, dtype=np.int32)
    lm[2, 10:10 + 1025] = 0
    lm[1, 20:24], lm[3:5, 30:33], lm[3, 1040] = 1, 2, 3
    got = check(lm, 4)
    assert got[2][0].tolist() == [0, 0, 0, 2] and got[3][0].tolist() == [0, 0, 0, 2] and got[4][0].tolist() == [0.0, 0.0]
    assert got[2][1:, 0].tolist() == [4, 4, 4] and got[2][1:, 3].tolist() == [0, 0, 0]
    lm[2, 10] = -1                                                                        # 1024 wide: measured
    got = check(lm, 4)
    assert got[2][0].tolist() == [4, 2 * 1024, 2 * 1025, 0] and got[3][0].tolist() == [4, 2 * 1024, 1024 * 1024 + 1, 0]


def test_garbage_extents_are_flagged_and_harmless():
    """valid entry points, valid buffers, extents that are not this map's: swapped between labels, negative, beyond the window, random, the
    whole window for everyone (the first row of the box is then rarely the label's first), the extremes of int32"""
    rng = np.random.default_rng(9)
    R, h, w = 7, 70, 150
    lm = mref.random_map(rng, h, w, R)
    own = mref.measure(lm, R)[1]
    seen = set()
    for g in (own[::-1].copy(), -own - 5, own + 1000, rng.integers(-3, w + 3, own.shape).astype(np.int32),
              np.tile(np.array([0, 0, w - 1, h - 1], dtype=np.int32), (R, 1)), rng.integers(-2 ** 31, 2 ** 31 - 1, own.shape).astype(np.int32),
              np.tile(np.array([-2 ** 31, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1], dtype=np.int64), (R, 1)).astype(np.int32),
              np.concatenate([own[:, :2], own[:, :2]], 1)):                               # the box shrunk to its corner pixel: the walk leaves it
        got = check(lm, R, g)
        seen |= set(got[2][:, 3].tolist()) | set(got[3][:, 3].tolist())
    assert {0, 1, 4} <= seen


def test_offsets_that_disagree_with_the_counts():
    rng = np.random.default_rng(10)
    R = 7
    lm = mref.random_map(rng, 33, 64, R)
    extent = mref.measure(lm, R)[1]
    offsets, verts, counts = ref.outlines(lm, R, extent)
    V = counts[:, 0]
    assert (V >= 4).sum() >= 3
    lm_d, ext_d = torch.from_numpy(lm).to(DEV), torch.from_numpy(extent).to(DEV)
    got, status = write_pass(lm_d, R, ext_d, torch.from_numpy(offsets).to(DEV))
    assert status == 0 and np.array_equal(got[:-TAIL].cpu().numpy(), verts) and bool((got[-TAIL:] == POISON).all())
    # every range one row short (ranges of 0 stay): the first V - 1 vertices of every label, nothing behind the last offset
    short = np.zeros(R + 1, dtype=np.int64)
    short[1:] = np.cumsum(np.maximum(V - 1, 0))
    got, status = write_pass(lm_d, R, ext_d, torch.from_numpy(short).to(DEV))
    want = np.concatenate([verts[offsets[r]:offsets[r + 1] - 1] for r in range(R) if V[r]])
    assert status == 1 and np.array_equal(got[:-TAIL].cpu().numpy(), want) and bool((got[-TAIL:] == POISON).all())
    # every range one row long: the last row of every range keeps its poison
    wide = np.zeros(R + 1, dtype=np.int64)
    wide[1:] = np.cumsum(V + 1)
    got, status = write_pass(lm_d, R, ext_d, torch.from_numpy(wide).to(DEV))
    got = got.cpu().numpy()
    assert status == 1 and (got[-TAIL:] == POISON).all()
    for r in range(R):
        assert np.array_equal(got[wide[r]:wide[r] + V[r]], verts[offsets[r]:offsets[r + 1]]) and (got[wide[r + 1] - 1] == POISON).all(), r
    # offsets that run backwards, below zero and beyond the total: nothing is written at all
    bad = offsets[::-1].copy()
    bad[0] = -3
    got, status = write_pass(lm_d, R, ext_d, torch.from_numpy(bad).to(DEV))
    assert status == 1 and bool((got == POISON).all())


def disc_map(overlap):
    """512 x 512, a disc per cell of pitch 24 with its centre moved by up to 2 pixels: radii 3 - 9 keep the discs apart; overlap: radii 8 - 16,
    later discs drawn over earlier ones, every fifth a ring around a background hole and every seventh a ring around another label"""
    rng = np.random.default_rng(11 + overlap)
    side, pitch = 512, 24
    lm = np.full((side, side), -1, dtype=np.int32)
    yy, xx = np.mgrid[0:side, 0:side]
    r = 0
    for cy in range(pitch // 2, side - pitch // 2 + 1, pitch):
        for cx in range(pitch // 2, side - pitch // 2 + 1, pitch):
            y, x = cy + int(rng.integers(-2, 3)), cx + int(rng.integers(-2, 3))
            rad = int(rng.integers(8, 17)) if overlap else int(rng.integers(3, 10))
            d2 = (yy - y) ** 2 + (xx - x) ** 2
            disc = d2 <= rad * rad
            if overlap and r % 5 == 0:
                disc &= d2 > (rad // 2) ** 2
            lm[disc] = r
            if overlap and r % 7 == 0:
                lm[d2 <= 4] = -1 if r % 2 else r + 1000
            r += 1
    return lm, r


@pytest.fixture(scope='module')
def discs():
    """the two disc maps and the restatement's answers: computed once, shared, never modified"""
    out = {}
    for overlap in (0, 1):
        lm, R = disc_map(overlap)
        extent = mref.measure(lm, R)[1]
        out[overlap] = dict(lm=lm, R=R, extent=extent, want=ref.outlines(lm, R, extent) + ref.hulls(lm, R, extent))
    return out


def test_discs_apart_are_all_simple(discs):
    case = discs[0]
    lm, R = case['lm'], case['R']
    assert R == 21 * 21
    check(lm, R, case['extent'], case['want'])
    lm_d = torch.from_numpy(lm).to(DEV)
    sums, extent = ops.label_measure(lm_d, R)
    assert np.array_equal(extent.cpu().numpy(), case['extent'])
    offsets, verts, counts = ops.label_outline(lm_d, R, extent)
    hull_i, hull_f = ops.label_hull(lm_d, R, extent)
    for g, w in zip((offsets, verts, counts, hull_i), case['want']):
        assert np.array_equal(g.cpu().numpy(), w)
    t = houtline.shape_table(sums, counts, hull_i, hull_f)
    assert all(v.device.type == 'cuda' for v in t.values())
    assert bool(t['simple'].all()) and torch.equal(t['outline_edges'], sums[:, 6]) and torch.equal(t['enclosed_area'], sums[:, 0])
    assert bool(((t['solidity'] > 0.75) & (t['solidity'] <= 1)).all()) and bool((t['feret_ratio'] > 0.8).all())
    assert bool(((t['convexity'] > 0.6) & (t['convexity'] <= 1)).all())
    for r in (0, 17, R - 1):
        row = ref.shape_row(int(sums[r, 0]), int(sums[r, 6]), case['want'][2][r], case['want'][3][r], case['want'][4][r])
        for k, v in row.items():
            np.testing.assert_allclose(float(t[k][r]), float(v), rtol=1e-9, err_msg=k)


def test_discs_overlapping_fragments_and_holes(discs):
    case = discs[1]
    got = check(case['lm'], case['R'], case['extent'], case['want'])
    n = mref.measure(case['lm'], case['R'])[0][:, 0]
    live = got[2][:, 3] == 0
    assert (got[2][live, 1] // 2 > n[live]).any() and (got[2][live, 1] // 2 < n[live]).any()          # holes enclosed; fragments left out


def test_ops_refuse_what_the_kernels_cannot_take():
    lm = torch.zeros((4, 4), dtype=torch.int32, device=DEV)
    ext = torch.zeros((1, 4), dtype=torch.int32, device=DEV)
    with pytest.raises(_lib.HdyError, match='int32'):
        ops.label_outline(lm.long(), 1, ext)
    with pytest.raises(_lib.HdyError, match='extent'):
        ops.label_hull(lm, 2, ext)
    with pytest.raises(_lib.HdyError, match='extent'):
        ops.label_outline(lm, 1, ext.long())
    _lib.dispatch_log(reset=True)
    offsets, verts, counts = ops.label_outline(lm, 0, ext[:0])
    hull_i, hull_f = ops.label_hull(lm, 0, ext[:0])
    assert offsets.tolist() == [0] and tuple(verts.shape) == (0, 2) and tuple(counts.shape) == (0, 4) and tuple(hull_i.shape) == (0, 4)
    assert tuple(hull_f.shape) == (0, 2) and _lib.dispatch_log() == []
    ext[0] = torch.tensor([0, 0, 3, 3])
    offsets, verts, counts = ops.label_outline(lm, 1, ext)
    ops.label_hull(lm, 1, ext)
    assert _lib.dispatch_log() == ['label_outline_count', 'label_outline_write', 'label_hull']
    assert offsets.tolist() == [0, 4] and verts.tolist() == [[0, 0], [4, 0], [4, 4], [0, 4]] and counts.tolist() == [[4, 32, 16, 0]]


def test_slide_end_to_end(mask_model, tmp_path):
    import evaluation
    _, dep = mask_model
    slide = synth_u8(256, 7).to(DEV)
    kw = dict(tile=128, overlap=32, batch_size=3, compute_masks=True, label_map=True, measure=True)
    evaluation.inference_on_slide(dep, slide, **kw)                                       # (warm: every plan and packing exists)
    _lib.dispatch_log(reset=True)
    plain = evaluation.inference_on_slide(dep, slide, **kw)['det']
    log_plain = _lib.dispatch_log(reset=True)
    off = evaluation.inference_on_slide(dep, slide, outlines=False, **kw)['det']
    log_off = _lib.dispatch_log(reset=True)
    got = evaluation.inference_on_slide(dep, slide, outlines=True, **kw)['det']
    log_on = _lib.dispatch_log()
    assert log_off == log_plain and not any('outline' in n or 'hull' in n for n in log_plain)
    assert [log_on.count(n) for n in ('label_outline_count', 'label_outline_write', 'label_hull')] == [1, 1, 1]
    assert [n for n in log_on if n not in ('label_outline_count', 'label_outline_write', 'label_hull')] == log_plain
    n = len(plain['boxes'])
    assert n > 0, 'the synthetic mask model found nothing on the slide: the test needs detections'
    assert list(off) == list(plain) and sorted(off['nuclei']) == sorted(plain['nuclei']) and 'polygons' not in plain
    assert sorted(got) == sorted(list(plain) + ['polygons']) and sorted(got['nuclei']) == sorted(list(plain['nuclei']) + list(houtline.SHAPE_COLUMNS))
    for k in plain:
        if k != 'nuclei':
            assert torch.equal(got[k], plain[k]) and torch.equal(off[k], plain[k]), k
    def same(a, b):
        return a.dtype == b.dtype and torch.equal(torch.nan_to_num(a.double(), nan=-1.0), torch.nan_to_num(b.double(), nan=-1.0))

    for k, v in plain['nuclei'].items():
        assert same(got['nuclei'][k], v) and same(off['nuclei'][k], v), k
    # the ops called by hand on the returned map
    lm = got['label_map']
    sums, extent = ops.label_measure(lm, n)
    offsets, verts, counts = ops.label_outline(lm, n, extent)
    hull_i, hull_f = ops.label_hull(lm, n, extent)
    assert torch.equal(got['polygons'][0], offsets) and torch.equal(got['polygons'][1], verts) and int(offsets[-1]) > 0
    want = houtline.shape_table(sums, counts, hull_i, hull_f)
    for k in houtline.SHAPE_COLUMNS:
        assert same(got['nuclei'][k], want[k]), k
    host = ref.outlines(lm.cpu().numpy(), n, extent.cpu().numpy())
    assert np.array_equal(host[0], offsets.cpu().numpy()) and np.array_equal(host[1], verts.cpu().numpy())
    path = str(tmp_path / 'nuclei.geojson')
    evaluation.save_polygons(path, got['polygons'], labels=got['labels'], scores=got['scores'])
    back = houtline.load_polygons(path)
    assert np.array_equal(back['rows'], np.nonzero(counts[:, 0].cpu().numpy())[0]) and np.array_equal(back['verts'], verts.cpu().numpy().astype(np.float64))
    with pytest.raises(ValueError, match='outlines=True needs measure=True'):
        evaluation.inference_on_slide(dep, slide, tile=128, overlap=32, batch_size=3, compute_masks=True, label_map=True, outlines=True)
