"""Mask paste on the MI355X (csrc/paste.hip and the layers above it): dense masks, the label map of a canvas or a window, the areas, and
evaluation.inference_on_slide(..., compute_masks=True, label_map=True).  Every comparison is bit for bit against the numpy restatement
(tests/paste_ref.py), which tests/test_paste_host.py ties to torch's own bilinear resize on the CPU."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import paste_ref as ref  # noqa: E402
from hd_yolo_amd import _lib, ops, synth  # noqa: E402

DEV = torch.device('cuda', 0)
W, H = 96, 80                                  # the canvas of the kernel cases
WINDOW = (17, 9, 50, 40)                       # (x0, y0, w, h): cuts boxes on all four sides
_CACHE = {}


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def integer_specs():
    """(bx1, by1, w, h) of the 37 boxes on the 96 x 80 canvas, as integer boxes after expansion"""
    spec = [
        (-6, 20, 14, 18), (88, 30, 20, 15), (30, -7, 22, 16), (40, 70, 19, 25),        # crossing the left, right, top and bottom border
        (-5, -4, 13, 12), (85, -6, 21, 17), (-8, 71, 18, 19), (87, 72, 23, 22),        # the four corners
        (130, 100, 20, 20),                                                            # wholly outside
        (-50, -35, 200, 150),                                                          # larger than the canvas
        (10, 10, 1, 1), (50, 33, 2, 7), (3, 40, 63, 5), (20, 50, 64, 9), (11, 60, 65, 3), (-100, 25, 300, 4),   # widths 1, 2, 63, 64, 65, > 256
        (-30, -25, 12, 11),                                                            # negative coordinates only: outside
        (60, 12, 5, 1), (70, 5, 1, 70), (0, 0, 96, 80), (95, 79, 1, 1), (0, 79, 3, 1),
    ]
    rng = np.random.default_rng(7)
    while len(spec) < 35:                                                              # seeded nucleus-sized boxes
        spec.append((int(rng.integers(-10, 90)), int(rng.integers(-10, 75)), int(rng.integers(6, 40)), int(rng.integers(6, 40))))
    return spec


def case(M, padding, cluster=False):
    """boxes fp32 (R, 4), masks fp32 (R, M, M): the 35 integer-placed boxes, a degenerate one and a NaN one (37), plus the cluster of eight"""
    key = (M, padding, cluster)
    if key not in _CACHE:
        spec = integer_specs()
        boxes = [ref.box_for(*s, M, padding) for s in spec]
        boxes.append([44.0, 22.0, 43.1, 21.3])                                          # degenerate: x2 < x1, y2 < y1
        boxes.append([float('nan'), 10.0, 30.0, 40.0])                                 # pastes nothing
        if cluster:
            rng = np.random.default_rng(11)
            for _ in range(8):                                                         # eight mutually overlapping masks around (48, 40)
                cx, cy = 48 + rng.uniform(-5, 5), 40 + rng.uniform(-5, 5)
                w, h = rng.uniform(18, 30, 2)
                boxes.append([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2])
        boxes = np.asarray(boxes, dtype=np.float32)
        rng = np.random.default_rng(100 + M)
        masks = np.stack([ref.ellipse_patch(rng, M) for _ in range(len(boxes))])
        _CACHE[key] = (boxes, masks)
    return _CACHE[key]


def label_case():
    """the 37 boxes and the cluster in ascending order of their integer area (NaN last): nucleus-sized boxes own their pixels before the
    canvas-sized ones, as rows in descending score order would; the reversed order is tested too"""
    boxes, masks = case(28, 1, cluster=True)
    ib, ok = ref.integer_boxes(boxes, 28, 1)
    area = np.where(ok, np.maximum(ib[:, 2] - ib[:, 0] + 1, 1) * np.maximum(ib[:, 3] - ib[:, 1] + 1, 1), 1 << 40)
    order = np.argsort(area, kind='stable')
    return boxes[order], masks[order]


def test_the_box_set_holds_what_it_claims():
    boxes, _ = case(28, 1)
    assert len(boxes) == 37
    ib, ok = ref.integer_boxes(boxes, 28, 1)
    assert ok.tolist() == [True] * 36 + [False]
    widths = (ib[:36, 2] - ib[:36, 0] + 1).tolist()
    assert all(w in widths for w in (1, 2, 63, 64, 65, 300, 200)) and widths[35] <= 0


def raw_dense(masks, boxes, size, padding):
    """hdy_paste_masks into a buffer pre-filled with NaN bytes (0xFF)"""
    R, M = masks.shape[0], masks.shape[-1]
    out = torch.full((R, size[0], size[1]), -1, dtype=torch.int32, device=DEV).view(torch.float32)
    assert torch.isnan(out).all()
    m, b = to_dev(masks), to_dev(boxes)
    _lib.call('hdy_paste_masks', m.data_ptr(), R, M, padding, b.data_ptr(), out.data_ptr(), out.numel(), size[0], size[1], ops.stream_ptr())
    return out


def same_bits(got, want):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype
    bad = got.view(np.int32) != want.view(np.int32)
    assert not bad.any(), f'{int(bad.sum())} of {bad.size} elements differ, first at {np.argwhere(bad)[:4].tolist()}'


@pytest.mark.parametrize('M', [28, 14])
@pytest.mark.parametrize('padding', [0, 1])
def test_dense_paste_equals_the_restatement(M, padding):
    boxes, masks = case(M, padding)
    want = ref.paste_masks(masks, boxes, (H, W), padding)
    assert want[:35].any(axis=(1, 2)).sum() >= 30 and not want[36].any()
    same_bits(raw_dense(masks, boxes, (H, W), padding), want)
    got = ops.paste_masks(to_dev(masks)[:, None], to_dev(boxes), (H, W), padding=padding)          # the (R, 1, M, M) form
    assert got.shape == (37, 1, H, W)
    same_bits(got[:, 0], want)


def test_dense_paste_walks_several_panels():
    """a clipped rectangle wider and taller than one 256 x 256 panel of the kernel's walk, and one that ends exactly on / one past a panel edge"""
    size = (270, 300)
    spec = [(-10, -20, 520, 600), (3, 5, 256, 256), (20, 7, 257, 258), (40, 260, 255, 30), (290, 100, 40, 40)]
    boxes = np.asarray([ref.box_for(*s, 28, 1) for s in spec], dtype=np.float32)
    rng = np.random.default_rng(5)
    masks = np.stack([ref.ellipse_patch(rng, 28) for _ in spec])
    same_bits(raw_dense(masks, boxes, size, 1), ref.paste_masks(masks, boxes, size, 1))
    lm = ops.paste_label_map(to_dev(masks), to_dev(boxes), size)
    want = ref.label_map(masks, boxes, (0, 0, size[1], size[0]))
    assert len(np.unique(want)) >= 4
    same_bits(lm, want)
    same_bits(ops.label_areas(lm, len(spec)), ref.areas(want, len(spec)))


@pytest.mark.parametrize('threshold', [0.5, 0.3])
@pytest.mark.parametrize('window', [None, WINDOW], ids=['canvas', 'window'])
def test_label_map_and_areas_equal_the_restatement(window, threshold):
    boxes, masks = label_case()
    R = len(boxes)
    assert R == 45
    x0, y0, w, h = window or (0, 0, W, H)
    want = ref.label_map(masks, boxes, (x0, y0, w, h), threshold)
    assert len(np.unique(want)) > 10 and ((want == -1).any() or window is not None)
    m, b = to_dev(masks), to_dev(boxes)
    # the raw entry point on a map pre-filled with garbage: it re-initialises the map itself
    lm = torch.randint(-5, 60, (h, w), dtype=torch.int32, device=DEV, generator=torch.Generator(DEV).manual_seed(3))
    _lib.call('hdy_paste_label_map', m.data_ptr(), R, 28, 1, b.data_ptr(), threshold, x0, y0, lm.data_ptr(), lm.numel(), h, w, ops.stream_ptr())
    same_bits(lm, want)
    want_areas = np.bincount(want[want >= 0], minlength=R).astype(np.int32)
    areas = torch.full((R,), 12345, dtype=torch.int32, device=DEV)                                # hdy_label_areas zeroes it itself
    _lib.call('hdy_label_areas', lm.data_ptr(), lm.numel(), areas.data_ptr(), R, ops.stream_ptr())
    same_bits(areas, want_areas)
    assert int(want_areas.sum()) == int((want >= 0).sum())
    # the Python surface, three repeats: bit-identical
    for _ in range(3):
        again = ops.paste_label_map(m, b, (H, W), window=window, threshold=threshold)
        assert again.dtype == torch.int32 and torch.equal(again, lm)
        assert torch.equal(ops.label_areas(again, R), areas)
    # the cluster: the lowest covering row owns a pixel, so reversing the rows changes owners but not the covered set
    rev = ops.paste_label_map(m.flip(0), b.flip(0), (H, W), window=window, threshold=threshold)
    assert torch.equal(rev >= 0, lm >= 0)
    same_bits(rev, ref.label_map(masks[::-1], boxes[::-1], (x0, y0, w, h), threshold))


def test_label_map_other_mask_sizes_and_padding():
    for M, padding in ((14, 1), (28, 0), (2, 1), (62, 1), (33, 0)):
        boxes, _ = label_case()
        rng = np.random.default_rng(M)
        masks = np.stack([ref.ellipse_patch(rng, M) for _ in range(len(boxes))])
        got = ops.paste_label_map(to_dev(masks), to_dev(boxes), (H, W), padding=padding)
        same_bits(got, ref.label_map(masks, boxes, (0, 0, W, H), 0.5, padding))


def test_empty_and_minimal_inputs():
    m0, b0 = torch.empty((0, 28, 28), device=DEV), torch.empty((0, 4), device=DEV)
    lm = ops.paste_label_map(m0, b0, (H, W))
    assert lm.shape == (H, W) and lm.dtype == torch.int32 and (lm == -1).all()
    areas = ops.label_areas(lm, 0)
    assert areas.shape == (0,) and areas.dtype == torch.int32
    assert ops.paste_masks(m0, b0, (H, W)).shape == (0, 1, H, W)
    assert ops.paste_masks(m0[:, None], b0, (H, W)).shape == (0, 1, H, W)
    # one detection on a 1 x 1 canvas
    masks = np.full((1, 28, 28), 0.9, dtype=np.float32)
    boxes = np.array([[-3.0, -2.0, 5.0, 4.0]], dtype=np.float32)
    lm = ops.paste_label_map(to_dev(masks), to_dev(boxes), (1, 1))
    same_bits(lm, ref.label_map(masks, boxes, (0, 0, 1, 1)))
    assert lm.tolist() == [[0]] and ops.label_areas(lm, 1).tolist() == [1]
    same_bits(ops.paste_masks(to_dev(masks), to_dev(boxes), (1, 1))[:, 0], ref.paste_masks(masks, boxes, (1, 1)))
    with pytest.raises(_lib.HdyError):
        ops.paste_label_map(to_dev(masks), to_dev(boxes), (H, W), window=(90, 0, 10, 10))         # leaves the canvas
    with pytest.raises(_lib.HdyError):
        ops.paste_masks(torch.zeros((1, 63, 63), device=DEV), to_dev(boxes), (H, W))


def test_label_map_beyond_2_31_entries():
    """a 46 342 x 46 342 map holds 2 147 580 964 entries, more than 2^31: the detections in its last rows are addressed correctly only in 64 bits"""
    side = 46342
    assert side * side > 2 ** 31
    spec = [(side - 40, side - 30, 35, 28), (side - 20, side - 60, 30, 30), (side - 90, side - 25, 50, 40), (5, 3, 20, 20)]
    boxes = np.asarray([ref.box_for(*s, 28, 1) for s in spec], dtype=np.float32)
    rng = np.random.default_rng(9)
    masks = np.stack([ref.ellipse_patch(rng, 28) for _ in spec])
    lm = ops.paste_label_map(to_dev(masks), to_dev(boxes), (side, side))
    tail = ref.label_map(masks, boxes, (side - 100, side - 100, 100, 100))
    head = ref.label_map(masks, boxes, (0, 0, 100, 100))
    assert (tail >= 0).sum() > 500 and (head == 3).any()
    same_bits(lm[side - 100:, side - 100:].contiguous(), tail)
    same_bits(lm[:100, :100].contiguous(), head)
    want = (ref.areas(tail, 4) + ref.areas(head, 4)).astype(np.int32)                   # every box lies inside one of the two corners
    same_bits(ops.label_areas(lm, 4), want)


# ---- end to end --------------------------------------------------------------------------------------------------------------------------
def mask_model():
    if 'model' not in _CACHE:
        from metayolo.models.yolo import Deploy, Model
        cfg = synth.make_cfg('n', 2)
        cfg['headers'][0][3][3] = 1                                       # the mask model of tests/test_gpu_slide.py / test_gpu_mask.py
        m = Model(cfg, synth.make_hyp(conf_thres=0.05))
        assert not m.load_state_dict(synth.mask_state_dict(m), strict=False).unexpected_keys
        m = m.to(DEV).eval()
        _CACHE['model'] = (m, Deploy(m))
    return _CACHE['model']


def synth_u8(size, seed):
    return (synth.synth_images(1, size, seed=seed)[0] * 255).round().to(torch.uint8).permute(1, 2, 0).contiguous()


@pytest.mark.parametrize('scale', [1.0, 0.5])
def test_slide_label_map_end_to_end(scale):
    import evaluation
    _, dep = mask_model()
    slide = synth_u8(256, 7).to(DEV)
    kw = dict(tile=128, overlap=32, batch_size=3, compute_masks=True, scale=scale)
    plain = evaluation.inference_on_slide(dep, slide, **kw)['det']
    got = evaluation.inference_on_slide(dep, slide, label_map=True, **kw)['det']
    n = len(plain['boxes'])
    print(f'scale {scale}: {n} detections')
    assert n > 0, 'the synthetic mask model found nothing on the slide: the test needs detections'
    assert sorted(got) == sorted(list(plain) + ['label_map', 'areas'])
    for k in ('boxes', 'scores', 'labels', 'masks'):
        assert got[k].dtype == plain[k].dtype and torch.equal(got[k], plain[k]), k
    side = int(round(256 * scale))
    assert got['label_map'].shape == (side, side) and got['label_map'].dtype == torch.int32 and got['areas'].shape == (n,)
    boxes, masks = got['boxes'].cpu().numpy(), got['masks'].cpu().numpy()[:, 0]
    want = ref.label_map(masks, boxes, (0, 0, side, side), 0.5, 1)
    same_bits(got['label_map'], want)
    same_bits(got['areas'], ref.areas(want, n))
    lm, areas = evaluation.slide_label_map(got, (side, side), window=(10, 20, 70, 60), threshold=0.3)
    want = ref.label_map(masks, boxes, (10, 20, 70, 60), 0.3, 1)
    same_bits(lm, want)
    same_bits(areas, ref.areas(want, n))


def test_label_map_needs_masks_and_a_mask_branch():
    import evaluation
    from metayolo.models.yolo import Deploy, Model
    _, dep = mask_model()
    slide = synth_u8(128, 7).to(DEV)
    with pytest.raises(ValueError, match='compute_masks'):
        evaluation.inference_on_slide(dep, slide, tile=128, overlap=0, batch_size=1, label_map=True)
    plain = Model(synth.make_cfg('n', 2), synth.make_hyp(conf_thres=0.05)).to(DEV).eval()
    with pytest.raises(ValueError, match='mask branch'):
        evaluation.inference_on_slide(Deploy(plain), slide, tile=128, overlap=0, batch_size=1, compute_masks=True, label_map=True)
    with pytest.raises(ValueError, match='masks'):
        evaluation.slide_label_map({'boxes': torch.zeros((0, 4), device=DEV)}, (8, 8))
