"""The label measurement on the MI355X (csrc/measure.hip: hdy_label_measure), through ops.label_measure, hd_yolo_amd/measure.py and
evaluation.inference_on_slide(..., label_map=True, measure=True).  sums and extent are compared bit for bit with the numpy restatement
(tests/measure_ref.py), which tests/test_measure_host.py ties to a per-label loop and to answers derived by hand."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import measure_ref as ref  # noqa: E402
from hd_yolo_amd import _lib, ops, synth  # noqa: E402
from hd_yolo_amd import measure as hmeasure  # noqa: E402
from test_gpu_mask_rows import mask_model  # noqa: E402,F401  (the module-scoped fixture)
from test_gpu_slide import synth_u8  # noqa: E402

DEV = torch.device('cuda', 0)


def run(lm, R, image=None, window=(0, 0), origin=None):
    """ops.label_measure on numpy inputs -> numpy outputs, and the same bits from the restatement"""
    img = None if image is None else (image if isinstance(image, torch.Tensor) else torch.from_numpy(image).to(DEV))
    org = None if origin is None else torch.from_numpy(origin).to(DEV)
    sums, extent = ops.label_measure(torch.from_numpy(lm).to(DEV), R, image=img, window=window, origin=org)
    assert sums.dtype == torch.int64 and tuple(sums.shape) == (R, 14) and extent.dtype == torch.int32 and tuple(extent.shape) == (R, 4)
    return sums.cpu().numpy(), extent.cpu().numpy()


def check(lm, R, image=None, window=(0, 0), origin=None):
    got = run(lm, R, image, window, origin)
    host_image = image.cpu().numpy() if isinstance(image, torch.Tensor) else image
    want = ref.measure(lm, R, host_image, window, origin)
    assert np.array_equal(got[0], want[0]), np.argwhere(got[0] != want[0])[:8]
    assert np.array_equal(got[1], want[1]), np.argwhere(got[1] != want[1])[:8]
    return got


@pytest.mark.parametrize('h,w', [(1, 1), (1, 63), (3, 65), (5, 130), (33, 64)])
def test_small_windows_cover_every_tile_edge(h, w):
    """widths that are no multiple of the wave or the tile (a run of one label goes on from the end of one map row into the start of the next:
    stripes of one label over whole rows), the halo at every tile edge, labels on every window border"""
    rng = np.random.default_rng(h * 1000 + w)
    R = 7
    image = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    lm = ref.random_map(rng, h, w, R)
    check(lm, R, image)
    stripes = np.repeat((np.arange(h, dtype=np.int32) // 2 % R)[:, None], w, 1)       # rows 2k and 2k + 1 hold one label from edge to edge
    got = check(stripes, R, image)
    assert int(got[0][0, 7]) > 0                                                      # label 0 lies on the top border
    check(np.zeros((h, w), dtype=np.int32), 1, image)                                 # one label everywhere: every edge is a border edge
    assert run(np.zeros((h, w), dtype=np.int32), 1)[0][0, :8].tolist()[6:] == [2 * (h + w), 2 * (h + w)]


def test_one_label_over_256_x_256_lands_on_one_row():
    rng = np.random.default_rng(1)
    image = rng.integers(0, 256, (256, 256, 3), dtype=np.uint8)
    got = check(np.full((256, 256), 2, dtype=np.int32), 3, image)
    assert got[0][2, 0] == 65536 and got[0][2, 6] == got[0][2, 7] == 1024 and got[1].tolist() == [[256, 256, -1, -1]] * 2 + [[0, 0, 255, 255]]
    assert int(got[0][2, 8]) == int(image[:, :, 0].astype(np.int64).sum()) and not got[0][:2].any()


@pytest.mark.parametrize('R', [4096, 100])
def test_every_entry_its_own_label(R):
    """64 x 64 with 4096 different values: 2048 labels per tile, more than any LDS table holds (most runs take the direct path to global
    memory); with R = 100 most of them are background and still count as different neighbours"""
    rng = np.random.default_rng(2)
    lm = rng.permutation(4096).astype(np.int32).reshape(64, 64)
    image = rng.integers(0, 256, (64, 64, 4), dtype=np.uint8)
    origin = rng.integers(-50, 50, (R, 2)).astype(np.int32)
    got = check(lm, R, image, (0, 0), origin)
    assert (got[0][:, 0] == 1).all() and (got[0][:, 6] == 4).all()


def test_non_labels_are_background_and_safe():
    R = 5
    lm = np.array([[-1, -7, 0x7fffffff, R, 0, 0, -(2 ** 31), R + 1], [4, 4, 4, R, 0x7fffffff, 2, 2, -1]], dtype=np.int32)
    got = check(lm, R)
    assert got[0][:, 0].tolist() == [2, 0, 2, 0, 3]
    big = np.random.default_rng(3).choice(np.array([-1, -7, 0x7fffffff, R], dtype=np.int64), size=(70, 150)).astype(np.int32)
    got = check(big, R)
    assert not got[0].any() and got[1].tolist() == [[150, 70, -1, -1]] * R


@pytest.fixture(scope='module')
def nuclei():
    """a 1024 x 1024 map of synthetic nuclei (synth.synth_slide_truth's detections, a disc pasted into every box by ops.paste_label_map), an
    RGBA slide around it, and the restatement's answer: computed once, shared, never modified"""
    side = 1024
    _, _, boxes, scores, _ = synth.synth_slide_truth(650, side, 3, seed=11)
    order = np.argsort(-scores, kind='stable')
    boxes = torch.from_numpy(boxes[order]).to(DEV)
    yy, xx = torch.meshgrid(torch.arange(28, device=DEV), torch.arange(28, device=DEV), indexing='ij')
    disc = (((yy - 13.5) ** 2 + (xx - 13.5) ** 2) <= 13.5 ** 2).float()
    lm = ops.paste_label_map(disc.expand(len(boxes), 28, 28), boxes, (side, side))
    rng = np.random.default_rng(4)
    rgba = rng.integers(0, 256, (side + 9, side + 40, 4), dtype=np.uint8)
    origin = boxes[:, :2].clamp(0, side - 1).to(torch.int32)
    case = dict(lm=lm, lm_host=lm.cpu().numpy(), R=len(boxes), boxes=boxes, rgba=rgba, origin=origin, origin_host=origin.cpu().numpy())
    case['want'] = ref.measure(case['lm_host'], case['R'], rgba, (17, 5), case['origin_host'])
    return case


def test_synthetic_nuclei_with_every_image_form(nuclei):
    lm, R, rgba = nuclei['lm_host'], nuclei['R'], nuclei['rgba']
    assert R > 500
    big = torch.from_numpy(rgba).to(DEV)
    # a crop view of a larger RGBA slide: row stride > w * 4, window origin (17, 5), alpha bytes random ("poison": never read)
    sums, extent = ops.label_measure(nuclei['lm'], R, image=big, window=(17, 5), origin=nuclei['origin'])
    want_s, want_e = nuclei['want']
    assert np.array_equal(sums.cpu().numpy(), want_s) and np.array_equal(extent.cpu().numpy(), want_e)
    assert torch.equal(sums[:, 0], ops.label_areas(nuclei['lm'], R).to(torch.int64)) and int(sums[:, 0].sum()) > 100000
    assert int((sums[:, 7] > 0).sum()) > 0                                                # nuclei cut by the window border
    # the same pixels as a crop view of the RGB slide (row stride > w * 3) whose view starts at the window: origin (0, 0)
    rgb = big[:, :, :3].contiguous()
    crop = rgb[5:5 + 1024, 17:17 + 1024]
    assert crop.stride(0) > 1024 * 3 and not crop.is_contiguous()
    s2, e2 = ops.label_measure(nuclei['lm'], R, image=crop, origin=nuclei['origin'])
    assert torch.equal(s2, sums) and torch.equal(e2, extent)
    # alpha bytes overwritten: nothing changes
    big2 = big.clone()
    big2[:, :, 3] = 0xA5
    s3, _ = ops.label_measure(nuclei['lm'], R, image=big2, window=(17, 5), origin=nuclei['origin'])
    assert torch.equal(s3, sums)
    # no image: the geometry is the same and the stain columns are zero
    s4, e4 = ops.label_measure(nuclei['lm'], R, origin=nuclei['origin'])
    assert torch.equal(s4[:, :8], sums[:, :8]) and not bool(s4[:, 8:].any()) and torch.equal(e4, extent)
    # no origin: moments about the window corner
    want0 = ref.measure(lm, R, None, (0, 0), None)
    s5, e5 = ops.label_measure(nuclei['lm'], R)
    assert np.array_equal(s5.cpu().numpy(), want0[0]) and np.array_equal(e5.cpu().numpy(), want0[1])
    with pytest.raises(_lib.HdyError, match='leaves the'):
        ops.label_measure(nuclei['lm'], R, image=big, window=(41, 5))


def test_origins_negative_and_large_enough_to_wrap():
    rng = np.random.default_rng(5)
    R = 9
    lm = ref.random_map(rng, 40, 200, R, labels_above=0)
    check(lm, R, None, (0, 0), rng.integers(-3000, 3000, (R, 2)).astype(np.int32))
    far = np.stack([np.full(R, -(2 ** 31)), np.full(R, 2 ** 31 - 1)], 1).astype(np.int32)
    got = check(lm, R, None, (0, 0), far)                      # dx^2 = 2^62 and more per entry: sum dx^2 wraps modulo 2^64, as numpy's int64 does
    exact = sum((int(j) + 2 ** 31) ** 2 for j in np.nonzero(lm == 0)[1])
    assert exact > 2 ** 64 and int(got[0][0, 3]) == (exact + 2 ** 63) % 2 ** 64 - 2 ** 63


def test_poisoned_outputs_and_repeats(nuclei, monkeypatch):
    """the call initialises both outputs itself (torch.empty is made to hand out poison), and three repeats are bit-identical"""
    R = nuclei['R']
    big = torch.from_numpy(nuclei['rgba']).to(DEV)
    real_empty = torch.empty

    def poisoned(*a, **k):
        t = real_empty(*a, **k)
        if t.dtype in (torch.int64, torch.int32):
            t.fill_(-0x5A5A5A5B)
        return t

    runs = []
    for _ in range(3):
        with monkeypatch.context() as mp:
            mp.setattr(torch, 'empty', poisoned)
            runs.append(ops.label_measure(nuclei['lm'], R, image=big, window=(17, 5), origin=nuclei['origin']))
    assert np.array_equal(runs[0][0].cpu().numpy(), nuclei['want'][0]) and np.array_equal(runs[0][1].cpu().numpy(), nuclei['want'][1])
    for s, e in runs[1:]:
        assert torch.equal(s, runs[0][0]) and torch.equal(e, runs[0][1])
    _lib.dispatch_log(reset=True)
    ops.label_measure(nuclei['lm'], R)
    assert _lib.dispatch_log() == ['label_measure']


def test_nucleus_table_on_the_device_equals_the_cpu_copy(nuclei):
    big = torch.from_numpy(nuclei['rgba']).to(DEV)
    sums, extent = ops.label_measure(nuclei['lm'], nuclei['R'], image=big, window=(17, 5), origin=nuclei['origin'])
    dev = hmeasure.nucleus_table(sums, extent, origin=nuclei['origin'], offset=(17, 5))
    cpu = hmeasure.nucleus_table(sums.cpu(), extent.cpu(), origin=nuclei['origin'].cpu(), offset=(17, 5))
    assert all(v.device.type == 'cuda' for v in dev.values()) and sorted(dev) == sorted(cpu)
    want = ref.table(sums.cpu().numpy(), extent.cpu().numpy(), nuclei['origin_host'], (17, 5))
    ref.assert_tables_agree({k: v.numpy() for k, v in cpu.items()}, want)
    ref.assert_tables_agree({k: v.cpu().numpy() for k, v in dev.items()}, want)
    own = cpu['area'] > 50
    # discs: nearly round, and the centroid lies inside the box it came from
    assert float(cpu['eccentricity'][own].median()) < 0.8 and float(cpu['compactness'][own].median()) > 0.5
    b = nuclei['boxes'].cpu().double()
    inside = (cpu['centroid_x'] - 17 >= b[:, 0] - 2) & (cpu['centroid_x'] - 17 <= b[:, 2] + 2) & (cpu['centroid_y'] - 5 >= b[:, 1] - 2) & \
        (cpu['centroid_y'] - 5 <= b[:, 3] + 2)
    assert bool(inside[own].all())


def test_wrapper_refuses_what_the_kernel_cannot_take():
    lm = torch.zeros((4, 4), dtype=torch.int32, device=DEV)
    with pytest.raises(_lib.HdyError, match='int32'):
        ops.label_measure(lm.long(), 1)
    with pytest.raises(_lib.HdyError, match='origin'):
        ops.label_measure(lm, 2, origin=torch.zeros((3, 2), dtype=torch.int32, device=DEV))
    with pytest.raises(_lib.HdyError, match='8-bit slide'):
        ops.label_measure(lm, 1, image=torch.zeros((3, 4, 4), dtype=torch.uint8, device=DEV).permute(1, 2, 0))
    s, e = ops.label_measure(lm, 0)
    assert tuple(s.shape) == (0, 14) and tuple(e.shape) == (0, 4)


def test_slide_end_to_end(mask_model):
    import evaluation
    _, dep = mask_model
    slide = synth_u8(256, 7).to(DEV)
    kw = dict(tile=128, overlap=32, batch_size=3, compute_masks=True, label_map=True)
    plain = evaluation.inference_on_slide(dep, slide, **kw)['det']
    _lib.dispatch_log(reset=True)
    again = evaluation.inference_on_slide(dep, slide, measure=False, **kw)['det']
    assert 'label_measure' not in _lib.dispatch_log()
    got = evaluation.inference_on_slide(dep, slide, measure=True, **kw)['det']
    assert _lib.dispatch_log().count('label_measure') == 1
    n = len(plain['boxes'])
    assert n > 0, 'the synthetic mask model found nothing on the slide: the test needs detections'
    assert 'nuclei' not in plain and 'nuclei' not in again and sorted(got) == sorted(list(plain) + ['nuclei'])
    for k in plain:
        assert got[k].dtype == plain[k].dtype and torch.equal(got[k], plain[k]) and torch.equal(again[k], plain[k]), k
    t = got['nuclei']
    assert torch.equal(t['area'], got['areas'].to(torch.int64)) and t['labels'] is got['labels'] and t['scores'] is got['scores']
    assert 'mean_rgb' in t and 'std_rgb' in t and t['mean_rgb'].shape == (n, 3)
    # the sums behind the table: measured again from the downloaded map and slide
    lm, img = got['label_map'].cpu().numpy(), slide.cpu().numpy()
    origin = np.minimum(np.maximum(np.nan_to_num(got['boxes'][:, :2].cpu().numpy()), 0), np.array([255, 255], dtype=np.float32)).astype(np.int32)
    sums, extent = ref.measure(lm, n, img, (0, 0), origin)
    ref.assert_tables_agree({k: v.cpu().numpy() for k, v in t.items()}, ref.table(sums, extent, origin, (0, 0)))
    s_dev, e_dev = ops.label_measure(got['label_map'], n, image=slide, origin=torch.from_numpy(origin).to(DEV))
    assert np.array_equal(s_dev.cpu().numpy(), sums) and np.array_equal(e_dev.cpu().numpy(), extent)
    # another magnification: the map and the slide no longer share a grid, so the table is morphology only
    half = evaluation.inference_on_slide(dep, slide, measure=True, scale=0.5, **kw)['det']
    assert 'nuclei' in half and 'mean_rgb' not in half['nuclei'] and 'std_rgb' not in half['nuclei']
    assert torch.equal(half['nuclei']['area'], half['areas'].to(torch.int64))
    with pytest.raises(ValueError, match='measure=True needs label_map=True'):
        evaluation.inference_on_slide(dep, slide, tile=128, overlap=32, batch_size=3, compute_masks=True, measure=True)
