"""Device mask rows on the MI355X: ops.roi_align_levels (hdy_roi_align_levels_fwd) against the per-level calls it replaces, ops.mask_rows
(hdy_mask_rows) against the indexing expression, Detect.masks_device against Detect.attach_masks on batches, and the masks of an 8-bit slide
beside the device append against the Python merge.  Every comparison is torch.equal; the switch HDY_DEVICE_MASKS is set explicitly."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from hd_yolo_amd import _lib, ops, synth  # noqa: E402
from test_gpu_kernels import DEV  # noqa: E402
from test_gpu_slide import expected, float_tiles, synth_u8  # noqa: E402

BF16, F32 = torch.bfloat16, torch.float32
INT_VIEW = {F32: torch.int32, BF16: torch.int16}


def bits(t):
    return t.contiguous().view(INT_VIEW[t.dtype])


# ------------------------------------------------------------------------------------------ roi_align_levels
B, MAX_DET, N_KEEP, P, C = 3, 8, [3, 0, 8], 14, 32
SIDES, STRIDES = [16, 8, 4], [8, 16, 32]                    # three levels of a 128 x 128 tile


def levels_case(dtype):
    g = torch.Generator().manual_seed(5)
    feats = []
    for side in SIDES:
        wide = torch.randn((B, side, side, 48), generator=g).to(dtype).to(DEV)
        feats.append(wide[..., 8:8 + C])                                        # a channel slice: pitch 48 > C
        assert feats[-1].stride(2) == 48 and not feats[-1].is_contiguous()
    xy = torch.rand((B, MAX_DET, 2), generator=g) * 90
    wh = torch.rand((B, MAX_DET, 2), generator=g) * 50 + 3
    boxes = torch.cat([xy, xy + wh], 2)
    boxes[0, 0] = torch.tensor([100.0, 100.0, 160.0, 170.0])                    # hangs over the map's edge
    boxes[0, 1] = torch.tensor([40.2, 40.3, 40.5, 41.0])                        # narrower than a pixel of every level
    boxes[2, 0] = torch.tensor([0.0, 0.0, 128.0, 128.0])                        # the whole map
    level = torch.tensor([[0, 2, 1, 0, 0, 0, 0, 0], [0] * 8, [1, 0, 0, 2, 1, 2, 0, 1]], dtype=torch.float32)
    for b, n in enumerate(N_KEEP):                                              # padded rows are scratch: NaN boxes, a level that does not exist
        boxes[b, n:] = float('nan')
        level[b, n:] = 99.0
    res = {'boxes': boxes.to(DEV).contiguous(), 'extra': level[:, :, None].to(DEV).contiguous(),
           'n_keep': torch.tensor(N_KEEP, dtype=torch.int32, device=DEV)}
    return feats, [1.0 / s for s in STRIDES], res


def per_level(feats, scales, res, n_keep, aligned):
    """Detect.attach_masks' assembly (yolo_head.py, the lines from `img = ...` to `torch.cat(parts)[order]`), restated"""
    dev = res['boxes'].device
    img = torch.cat([torch.full((n,), float(b), device=dev) for b, n in enumerate(n_keep)])
    boxes = torch.cat([res['boxes'][b, :n] for b, n in enumerate(n_keep)])
    levels = torch.cat([res['extra'][b, :n, 0] for b, n in enumerate(n_keep)]).long()
    rois = torch.cat([img[:, None], boxes], 1)
    parts, pos = [], []
    for l in range(len(feats)):
        sel = (levels == l).nonzero().flatten()
        pos.append(sel)
        parts.append(ops.roi_align(feats[l], rois[sel], scales[l], P, 2, aligned))
    order = torch.empty(len(rois), dtype=torch.long, device=dev)
    order[torch.cat(pos)] = torch.arange(len(rois), device=dev)
    return torch.cat(parts)[order].contiguous()


@pytest.mark.parametrize('aligned', [False, True], ids=['legacy', 'aligned'])
@pytest.mark.parametrize('dtype', [F32, BF16], ids=['fp32', 'bf16'])
def test_roi_align_levels_equals_the_per_level_calls(dtype, aligned):
    feats, scales, res = levels_case(dtype)
    total = sum(N_KEEP)
    want = per_level(feats, scales, res, N_KEEP, aligned)
    assert want.shape == (total, P, P, C) and bool(want.float().abs().sum() > 0) and bool(torch.isfinite(want.float()).all())
    canary = 123.0
    out = torch.full((total + 2, P, P, C), canary, dtype=dtype, device=DEV)
    _lib.dispatch_log(reset=True)
    got = ops.roi_align_levels(feats, scales, res, total + 2, P, 2, aligned, out=out)
    assert _lib.dispatch_log() == ['roi_align_levels']
    assert got is out and torch.equal(bits(got[:total]), bits(want))
    assert torch.equal(got[total:], torch.full_like(got[total:], canary)), 'rows behind the total were written'
    # a fresh buffer of exactly the total, as Detect.masks_device asks for it
    assert torch.equal(bits(ops.roi_align_levels(feats, scales, res, total, P, 2, aligned)), bits(want))
    # fewer rows than the total: the first out_rows rows, nothing else
    out = torch.full((5, P, P, C), canary, dtype=dtype, device=DEV)
    ops.roi_align_levels(feats, scales, res, 4, P, 2, aligned, out=out[:4])
    assert torch.equal(bits(out[:4]), bits(want[:4])) and torch.equal(out[4:], torch.full_like(out[4:], canary))
    # a valid row whose level does not exist writes zeros; every other row keeps its bits
    res['extra'][2, 3, 0] = 7.0
    row = N_KEEP[0] + N_KEEP[1] + 3
    again = ops.roi_align_levels(feats, scales, res, total, P, 2, aligned)
    assert not bool(again[row].any()) and bool(want[row].any())
    others = [r for r in range(total) if r != row]
    assert torch.equal(bits(again[others]), bits(want[others]))
    res['extra'][2, 3, 0] = float('nan')                                       # not finite: zeros too
    assert not bool(ops.roi_align_levels(feats, scales, res, total, P, 2, aligned)[row].any())


# ------------------------------------------------------------------------------------------ mask_rows
def test_mask_rows_equals_the_indexing_expression():
    R, M, K = 5, 28, 3
    g = torch.Generator().manual_seed(3)
    wide = torch.rand((R, M, M, 8), generator=g).to(DEV)
    vals = wide[..., :K]                                                        # K = 3 inside pitch 8
    table = torch.tensor([2, -1, 0, 1], dtype=torch.int32, device=DEV)
    labels = torch.tensor([0, 1, -1, 3, 2], dtype=torch.int64, device=DEV)
    m = vals.permute(0, 3, 1, 2)
    idx = table.long()[labels.clamp(min=0)]
    want = m[torch.arange(R, device=DEV), idx][:, None].clone()
    want[idx < 0] = 0
    got = ops.mask_rows(vals, labels, table, host_indices=[2, -1, 0, 1])
    assert got.shape == (R, 1, M, M) and got.is_contiguous() and torch.equal(bits(got), bits(want))
    assert not bool(got[1].any()) and torch.equal(got[2, 0], vals[2, :, :, 2]) and torch.equal(got[3, 0], vals[3, :, :, 1])
    assert torch.equal(bits(ops.mask_rows(vals, labels, table)), bits(want))                  # without the host copy of the table
    # what the host cannot see writes zeros: a label behind the table, an index behind the channels (device-only table)
    far = ops.mask_rows(vals, torch.tensor([0, 9, 0, 0, 0], dtype=torch.int64, device=DEV), table)
    assert not bool(far[1].any()) and torch.equal(far[0], want[0])
    wrong = ops.mask_rows(vals, labels, torch.tensor([5, -1, 0, 1], dtype=torch.int32, device=DEV))
    assert not bool(wrong[0].any()) and torch.equal(wrong[3:], want[3:])
    with pytest.raises(_lib.HdyError, match='mask channels'):
        ops.mask_rows(vals, labels, table, host_indices=[2, -1, 0, 3])
    empty = ops.mask_rows(wide[:0, :, :, :K], labels[:0], table)
    assert empty.shape == (0, 1, M, M) and empty.dtype == torch.float32


# ------------------------------------------------------------------------------------------ batches and whole slides
@pytest.fixture(scope='module')
def mask_model():
    """the mask model of tests/test_gpu_slide.py::test_masks_keep_the_python_merge_on_gathered_tiles: variant n, one mask class, fp32"""
    from metayolo.models.yolo import Deploy, Model
    cfg = synth.make_cfg('n', 2)
    cfg['headers'][0][3][3] = 1
    m = Model(cfg, synth.make_hyp(conf_thres=0.05))
    assert not m.load_state_dict(synth.mask_state_dict(m), strict=False).unexpected_keys
    m = m.to(DEV).eval()
    return m, Deploy(m)


def boom(what):
    def raiser(*a, **k):
        raise AssertionError(f'{what} was reached')
    return raiser


def test_batches_agree_with_attach_masks(mask_model, monkeypatch):
    from metayolo.models.yolo_head import Detect
    m, dep = mask_model
    x = float_tiles(synth_u8(256, 7), [(0, 0), (128, 0), (0, 128)], 128, 128).to(DEV)
    monkeypatch.setenv('HDY_DEVICE_MASKS', '0')
    _, want = dep(x, compute_masks=True)
    monkeypatch.setenv('HDY_DEVICE_MASKS', '1')
    dep(x, compute_masks=True)                                                  # (warm: every plan and packing exists)
    _lib.dispatch_log(reset=True)
    with monkeypatch.context() as mp:
        mp.setattr(Detect, 'attach_masks', boom('Detect.attach_masks'))         # the parent commit's only route to masks
        _, got = dep(x, compute_masks=True)
    log = _lib.dispatch_log()
    assert log.count('roi_align_levels') == 1 and log.count('mask_rows') == 1 and 'roi_align' not in log, [n for n in log if 'roi' in n or 'mask' in n]
    assert len(got) == len(want) == 3
    total = 0
    for g, w in zip(got, want):
        g, w = g['det'], w['det']
        assert list(g) == list(w), (list(g), list(w))
        assert ('masks' in w) == (len(w['boxes']) > 0)
        for k in w:
            assert g[k].dtype == w[k].dtype and g[k].shape == w[k].shape and torch.equal(g[k], w[k]), k
        total += len(w['boxes'])
    print(f'batch of 3 tiles: {[len(w["det"]["boxes"]) for w in want]} detections')
    assert total > 0


SLIDES = {'tail_chunk': (256, 7, 128, 0, 3),                 # 4 tiles: chunks of 3 and 1
          'overlap': (320, 7, 128, 64, 4)}                   # 16 tiles, the slide NMS drops rows: the masks follow `keep`


@pytest.mark.parametrize('name', list(SLIDES))
def test_whole_slide_masks_travel_beside_the_append(name, mask_model, monkeypatch):
    import evaluation
    from metayolo.models.yolo_head import Detect
    m, dep = mask_model
    size, seed, tile, overlap, bs = SLIDES[name]
    slide = synth_u8(size, seed).to(DEV)
    kw = dict(tile=tile, overlap=overlap, batch_size=bs, compute_masks=True, label_map=True)
    nms_rows, nms = [], evaluation.nms

    def spy_nms(boxes, scores, thr):
        keep = nms(boxes, scores, thr)
        nms_rows.append((len(boxes), len(keep)))
        return keep

    monkeypatch.setattr(evaluation, 'nms', spy_nms)
    monkeypatch.setenv('HDY_DEVICE_MASKS', '0')
    want = evaluation.inference_on_slide(dep, slide, **kw)['det']
    recipe = expected(dep, m.headers['det'], slide, tile, overlap, bs, compute_masks=True)
    monkeypatch.setenv('HDY_DEVICE_MASKS', '1')
    del nms_rows[:]
    with monkeypatch.context() as mp:
        mp.setattr(Detect, 'merge_outputs', boom('Detect.merge_outputs'))
        mp.setattr(Detect, 'attach_masks', boom('Detect.attach_masks'))
        runs = [evaluation.inference_on_slide(dep, slide, **kw)['det'] for _ in range(3)]
    got = runs[0]
    print(f'{name}: {len(want["boxes"])} detections, slide NMS (before, after) = {nms_rows}')
    assert len(want['boxes']) > 0
    if overlap:
        assert len(nms_rows) == 3 and all(0 < after < before for before, after in nms_rows), nms_rows
    keys = ['boxes', 'scores', 'labels', 'masks', 'label_map', 'areas']
    assert sorted(got) == sorted(want) == sorted(keys)
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and torch.equal(got[k], want[k]), k
    for k in keys[:4]:
        assert torch.equal(got[k], recipe[k]), f'{k} differs from the float recipe'
    assert got['masks'].shape[1:] == (1, 28, 28) and bool((got['label_map'] >= 0).any())
    for again in runs[1:]:
        for k in keys:
            assert torch.equal(again[k], got[k]), f'{k} differs between repeats'


def test_slide_without_detections_keeps_the_keys_of_the_python_merge(mask_model, monkeypatch):
    """conf_thres above every score of the synthetic weights (they stay below 0.6): no tile detects anything; the keys are those of
    _zero_row_masks + merge_outputs on the same slide"""
    import evaluation
    m, dep = mask_model
    slide = synth_u8(256, 7).to(DEV)
    monkeypatch.setitem(m.headers['det'].nms_params, 'conf_thres', 0.9)
    for label_map in (True, False):
        kw = dict(tile=128, overlap=0, batch_size=3, compute_masks=True, label_map=label_map)
        monkeypatch.setenv('HDY_DEVICE_MASKS', '0')
        want = evaluation.inference_on_slide(dep, slide, **kw)['det']
        monkeypatch.setenv('HDY_DEVICE_MASKS', '1')
        got = evaluation.inference_on_slide(dep, slide, **kw)['det']
        assert len(want['boxes']) == 0 and sorted(got) == sorted(want) and ('masks' in want) == label_map
        for k in want:
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and torch.equal(got[k], want[k]), k
