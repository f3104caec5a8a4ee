"""8-bit whole-slide inference on the MI355X (csrc/slide.hip and the layers above it): tile gather, result append, tissue counts, and
evaluation.inference_on_slide on uint8 HWC slides against an expectation made here from the float path's own pieces.  Everything is compared
with torch.equal.  The pixel table is made on the CPU: float(v) / 255 correctly rounded is the contract, what a device division does is not."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hd_yolo_amd import _lib, ops, synth  # noqa: E402
from test_gpu_kernels import DEV  # noqa: E402

TABLE = torch.arange(256).float() / 255              # on the CPU
BF16, F32 = torch.bfloat16, torch.float32
INT_VIEW = {torch.float32: torch.int32, torch.bfloat16: torch.int16}
PATTERNS = {torch.int32: (0, -1, 0x7F7F7F7F), torch.int16: (0, -1, 0x7F7F)}      # the three fills of tests/test_gpu_scratch.py


def bits(t):
    return t.view(INT_VIEW[t.dtype])


def float_tiles(slide, origins, th, tw):
    """(n, 3, th, tw) float tiles table[v] of a CPU uint8 (H, W, C) slide, zero where a window lies outside the slide"""
    H, W, _ = slide.shape
    x = torch.zeros((len(origins), 3, th, tw))
    for j, (x0, y0) in enumerate(origins):
        ys, xs = max(y0, 0), max(x0, 0)
        ye, xe = min(y0 + th, H), min(x0 + tw, W)
        if ye > ys and xe > xs:
            x[j, :, ys - y0:ye - y0, xs - x0:xe - x0] = TABLE[slide[ys:ye, xs:xe, :3].long()].permute(2, 0, 1)
    return x


def u8(shape, seed):
    return torch.randint(0, 256, shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


def slides():
    big = u8((300, 411, 3), 3)
    big4 = u8((220, 333, 4), 4)
    return {
        'rgb_odd': u8((150, 203, 3), 1).to(DEV),                         # W * 3 = 609: rows start at every byte phase
        'rgba_odd': u8((97, 131, 4), 2).to(DEV),
        'rgb_view': big.to(DEV)[13:213, 5:306],                          # a crop of a larger slide: pitch 1233, odd base offset
        'rgba_view': big4.to(DEV)[7:207, 3:300],
        'rgb_small': u8((50, 70, 3), 5).to(DEV),                         # smaller than the tile
    }


def border_origins(H, W, th, tw):
    o = [(0, 0), (max(W - tw, 0), 0), (0, max(H - th, 0)), (max(W - tw, 0), max(H - th, 0)), (W // 3, H // 4), (1, 2), (3, 1),
         (W - tw // 2, H - th // 3), (-5, -7), (W + 3, 0)]               # the last three hang over the slide's edges / lie outside
    return o


@pytest.mark.parametrize('dtype', [BF16, F32], ids=['bf16', 'fp32'])
@pytest.mark.parametrize('name', ['rgb_odd', 'rgba_odd', 'rgb_view', 'rgba_view', 'rgb_small'])
@pytest.mark.parametrize('th,tw', [(64, 72), (40, 63)])
def test_gather_equals_stem_prep_and_nhwc_of_the_float_tiles(name, dtype, th, tw):
    slide = slides()[name]
    H, W, _ = slide.shape
    origins = border_origins(H, W, th, tw)
    first, count = 1, len(origins) - 1
    table = ops.slide_origins(origins, DEV)
    x = float_tiles(slide.cpu(), origins[first:first + count], th, tw).to(DEV)
    iv = INT_VIEW[dtype]
    # stem layout: count tiles, one spare tile behind them
    want = torch.empty((count, th + 4, tw + 4, 4), dtype=dtype, device=DEV)
    ops.run([ops.rec_stem_prep(x, want)])
    assert (want[:, :2] == 0).all() and (want[:, -2:] == 0).all() and (want[:, :, :2] == 0).all() and (want[:, :, -2:] == 0).all()
    assert (want[..., 3] == 0).all()
    _lib.dispatch_log(reset=True)
    for pat in PATTERNS[iv]:
        buf = torch.empty((count + 1, th + 4, tw + 4, 4), dtype=dtype, device=DEV)
        bits(buf).fill_(pat)
        ops.run([ops.rec_slide_tiles(slide, table, first, count, buf[:count])])
        assert torch.equal(bits(buf[:count]), bits(want)), (name, pat)
        assert (bits(buf[count]) == pat).all(), 'bytes behind the count tiles were touched'
    assert 'slide_tiles_u8_stem' in _lib.dispatch_log()
    # pitched NHWC: channels 0..2 of an 8-wide pixel, the other lanes keep the fill on both sides
    for pat in PATTERNS[iv]:
        ref = torch.empty((count + 1, th, tw, 8), dtype=dtype, device=DEV)
        got = torch.empty((count + 1, th, tw, 8), dtype=dtype, device=DEV)
        bits(ref).fill_(pat)
        bits(got).fill_(pat)
        ops.run([ops.rec_nchw_to_nhwc(x, ref[:count, ..., :3])])
        ops.run([ops.rec_slide_tiles(slide, table, first, count, got[:count, ..., :3], pad=0)])
        assert torch.equal(bits(got), bits(ref)), (name, pat)
    assert 'slide_tiles_u8_nhwc' in _lib.dispatch_log()


def test_gather_addresses_a_slide_of_more_than_4_gb():
    """38 000 x 38 000 x 3 = 4.33 GB: the first tile, one straddling byte offset 2^32 and the last.  Allocated once, freed before the next test."""
    S, th, tw = 38000, 64, 64
    slide = torch.empty((S, S, 3), dtype=torch.uint8, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(11)
    for r in range(0, S, 2000):
        slide[r:r + 2000] = torch.randint(0, 256, (min(2000, S - r), S, 3), dtype=torch.uint8, device=DEV, generator=g)
    pitch = S * 3
    y_mid, x_mid = (1 << 32) // pitch, ((1 << 32) % pitch) // 3
    origins = [(0, 0), (max(x_mid - tw // 2, 0), y_mid - th // 2), (S - tw, S - th)]
    first_byte = origins[1][1] * pitch + origins[1][0] * 3
    last_byte = (origins[1][1] + th - 1) * pitch + (origins[1][0] + tw) * 3
    assert first_byte < (1 << 32) < last_byte and (S - th) * pitch > (1 << 32)
    crops = [slide[y0:y0 + th, x0:x0 + tw].cpu() for x0, y0 in origins]
    x = torch.stack([TABLE[c.long()].permute(2, 0, 1) for c in crops]).to(DEV)
    try:
        for dtype in (BF16, F32):
            want = torch.empty((3, th + 4, tw + 4, 4), dtype=dtype, device=DEV)
            got = torch.empty_like(want)
            bits(got).fill_(-1)
            ops.run([ops.rec_stem_prep(x, want)])
            ops.run([ops.rec_slide_tiles(slide, ops.slide_origins(origins, DEV), 0, 3, got)])
            assert torch.equal(bits(got), bits(want)), dtype
        counts = ops.slide_tissue(slide, ops.slide_origins(origins, DEV), th, tw, 128).cpu()
        want_c = [int((c.min(dim=2).values < 128).sum()) for c in crops]
        assert counts.tolist() == want_c
    finally:
        del slide
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------ append
def _parts(n_keep, origins, seed):
    """compacted detections of one batch and the per-tile dicts Detect.merge_outputs takes"""
    g = torch.Generator().manual_seed(seed)
    total, max_det = sum(n_keep), max(max(n_keep), 1)
    rows = len(n_keep) * max_det                                          # det_outputs' arrays: bs * max_det rows, scratch past the total
    boxes = torch.rand((rows, 4), generator=g) * 640
    scores = torch.rand((rows,), generator=g)
    labels = torch.randint(-100, 9, (rows,), generator=g)
    parts, at = [], 0
    for n, (x0, y0) in zip(n_keep, origins):
        parts.append({'boxes': boxes[at:at + n].to(DEV), 'scores': scores[at:at + n].to(DEV), 'labels': labels[at:at + n].to(DEV),
                      'roi': (float(x0), float(y0))})
        at += n
    assert at == total
    return (boxes.to(DEV), scores.to(DEV), labels.to(DEV), torch.tensor(n_keep, dtype=torch.int32, device=DEV)), parts


def _accumulators(cap, spare=5):
    big = (torch.full((cap + spare, 4), -7.0, device=DEV), torch.full((cap + spare,), -7.0, device=DEV),
           torch.full((cap + spare,), -7, dtype=torch.int64, device=DEV))
    return big, tuple(t[:cap] for t in big), torch.zeros((2,), dtype=torch.int32, device=DEV)


def test_append_equals_merge_outputs():
    from metayolo.models.yolo_head import Detect
    max_det = 7
    origins = [(0, 0), (576, 0), (1152, 0), (19360, 0), (0, 576), (576, 576), (33, 19360), (19360, 19360), (5, 5), (100000, 70000), (1, 2)]
    table = ops.slide_origins(origins, DEV)
    batches = [([3, 0, max_det, 0, 2], 0), ([0, 0, 0], 5), ([1, max_det, 4], 8)]      # empty tiles, a full tile, an all-empty batch
    big, acc, cursor = _accumulators(len(origins) * max_det)
    all_parts = []
    for k, (n_keep, first) in enumerate(batches):
        dev, parts = _parts(n_keep, origins[first:first + len(n_keep)], seed=20 + k)
        ops.slide_append(*dev, table, first, *acc, cursor)
        all_parts += parts
    want = Detect.merge_outputs(None, all_parts)
    rows, overflow = cursor.tolist()
    assert overflow == 0 and rows == len(want['boxes']) == 24
    assert torch.equal(acc[0][:rows], want['boxes']) and torch.equal(acc[1][:rows], want['scores']) and torch.equal(acc[2][:rows], want['labels'])
    assert (acc[0][rows:] == -7).all() and (acc[1][rows:] == -7).all() and (acc[2][rows:] == -7).all()
    # repeats on fresh accumulators: bit-identical
    for _ in range(3):
        _, acc2, cursor2 = _accumulators(len(origins) * max_det)
        for k, (n_keep, first) in enumerate(batches):
            dev, _p = _parts(n_keep, origins[first:first + len(n_keep)], seed=20 + k)
            ops.slide_append(*dev, table, first, *acc2, cursor2)
        assert cursor2.tolist() == [rows, 0]
        assert all(torch.equal(a, b) for a, b in zip(acc2, acc))


def test_append_raises_the_overflow_flag_instead_of_writing_past_the_end():
    from metayolo.models.yolo_head import Detect
    origins = [(10, 20), (30, 40), (50, 60), (70, 80)]
    table = ops.slide_origins(origins, DEV)
    dev1, parts1 = _parts([4, 2], origins[:2], seed=1)
    dev2, parts2 = _parts([3, 5], origins[2:], seed=2)
    cap = 4 + 2 + 3 + 5 - 1                                               # one row short
    big, acc, cursor = _accumulators(cap)
    ops.slide_append(*dev1, table, 0, *acc, cursor)
    assert cursor.tolist() == [6, 0]
    ops.slide_append(*dev2, table, 2, *acc, cursor)
    assert cursor.tolist() == [cap, 1]
    want = Detect.merge_outputs(None, parts1 + parts2)
    assert torch.equal(acc[0], want['boxes'][:cap]) and torch.equal(acc[1], want['scores'][:cap]) and torch.equal(acc[2], want['labels'][:cap])
    assert (big[0][cap:] == -7).all() and (big[1][cap:] == -7).all() and (big[2][cap:] == -7).all(), 'rows behind the capacity were written'
    ops.slide_append(*dev1, table, 0, *acc, cursor)                       # a full array takes nothing more, the flag stays
    assert cursor.tolist() == [cap, 1] and torch.equal(acc[0], want['boxes'][:cap])


# ------------------------------------------------------------------------------------------ tissue counts
def tissue_ref(slide, table, th, tw, background):
    t = slide[:, :, :3].min(axis=2) < background
    H, W = t.shape
    return [int(t[max(y0, 0):max(min(y0 + th, H), 0), max(x0, 0):max(min(x0 + tw, W), 0)].sum()) for x0, y0 in table]


@pytest.mark.parametrize('channels', [3, 4])
def test_tissue_counts_equal_numpy(channels):
    rng = np.random.default_rng(7)
    H, W, th, tw = 301, 415, 96, 100
    s = rng.integers(0, 256, (H, W, channels), dtype=np.uint8)
    s[:100, 200:] = 255                                                   # blank
    s[100:200, :150] = rng.integers(0, 100, (100, 150, channels), dtype=np.uint8)      # full
    s[200:, 100:300, :3] = 240                                            # light: background at 220, tissue at 255
    s[250:, 300:] = 220                                                   # exactly the default threshold: background
    origins = [(200, 0), (300, 2), (0, 100), (50, 104), (150, 50), (100, 200), (130, 205), (315, 205), (310, 250), (-20, -30), (400, 290), (500, 0)]
    big = torch.from_numpy(np.pad(s, ((3, 2), (5, 7), (0, 0)))).to(DEV)
    for slide in (torch.from_numpy(s).to(DEV), big[3:3 + H, 5:5 + W]):    # contiguous, and a view with a larger pitch
        table = ops.slide_origins(origins, DEV)
        for background in (0, 220, 255):
            got = ops.slide_tissue(slide, table, th, tw, background)
            assert got.dtype == torch.int32 and got.tolist() == tissue_ref(s, origins, th, tw, background), background
    assert ops.slide_tissue(torch.from_numpy(s).to(DEV), table, th, tw, 0).sum().item() == 0


# ------------------------------------------------------------------------------------------ whole slide
def _model(half, multi_label=False):
    from metayolo.models.yolo import Deploy, Model
    m = Model(synth.make_cfg('n', 3), synth.make_hyp(conf_thres=0.05, multi_label=multi_label)).to(DEV).eval()
    m.load_state_dict(synth.synth_state_dict(synth.shapes_of(m), seed=2), strict=False)
    if half:
        m.half()
    return m, Deploy(m)


def synth_u8(size, seed, alpha=False):
    """(synth_images * 255).round() as the uint8 HWC tensor a slide reader delivers"""
    s = (synth.synth_images(1, size, seed=seed)[0] * 255).round().to(torch.uint8).permute(1, 2, 0).contiguous()
    if alpha:
        s = torch.cat([s, u8((size, size, 1), seed + 100)], 2).contiguous()
    return s


def expected(dep, header, slide, tile, overlap, batch_size, scale=1.0, origins=None, compute_masks=False):
    """The float path's recipe (tests/test_gpu_f3.py::test_inference_on_slide_merges_rois) on the tiles table[v]: per chunk dep(x), boxes
    shifted by the origin, concatenated; ops.nms when the windows overlap; clamp; scale."""
    import evaluation
    H, W, _ = slide.shape
    flt = TABLE.to(DEV)[slide[:, :, :3].long()].permute(2, 0, 1)          # a gather from the CPU-made table: exact
    rois = evaluation.slide_rois(H, W, tile, overlap) if origins is None else [tuple(o) for o in origins]
    parts = {'boxes': [], 'scores': [], 'labels': [], 'masks': []}
    for i in range(0, len(rois), batch_size):
        chunk = rois[i:i + batch_size]
        x = torch.zeros((len(chunk), 3, tile, tile), device=DEV)
        for j, (x0, y0) in enumerate(chunk):
            patch = flt[:, y0:y0 + tile, x0:x0 + tile]
            x[j, :, :patch.shape[1], :patch.shape[2]] = patch
        _, outs = dep(x, compute_masks=compute_masks)
        for (x0, y0), o in zip(chunk, outs):
            o = o['det']
            parts['boxes'].append(o['boxes'] + torch.tensor([x0, y0, x0, y0], device=DEV, dtype=torch.float32))
            parts['scores'].append(o['scores'])
            parts['labels'].append(o['labels'])
            if 'masks' in o:
                parts['masks'].append(o['masks'])
    r = {k: torch.cat(v) for k, v in parts.items() if v}
    if len(r['boxes']) and overlap > 0:
        keep = ops.nms(r['boxes'], r['scores'], header.nms_params['iou_thres'])
        r = {k: v[keep] for k, v in r.items()}
    r['boxes'][:, [0, 2]] = r['boxes'][:, [0, 2]].clamp(0, W)
    r['boxes'][:, [1, 3]] = r['boxes'][:, [1, 3]].clamp(0, H)
    r['boxes'] = r['boxes'] * scale
    return r


def assert_same(got, want, what=''):
    print(f'{what}: {len(want["boxes"])} detections expected, {len(got["boxes"])} found')
    assert sorted(got) == sorted(want), (what, sorted(got), sorted(want))
    for k in want:
        assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), (what, k)
    assert len(want['boxes']) > 0, what


def slide_case(name):
    """(8-bit slide on the device, tile, overlap, batch_size, scale, nms grid minimum or None)"""
    if name == 'tail_chunk':
        return synth_u8(256, 9).to(DEV), 128, 0, 3, 0.5, None            # 4 tiles: chunks of 3 and 1
    if name == 'overlap_grid':
        return synth_u8(448, 9).to(DEV), 128, 64, 12, 1.0, 256           # 36 tiles, merged through nms_grid
    if name == 'crop_view':
        return synth_u8(320, 4).to(DEV)[60:260, 10:310], 128, 32, 4, 1.0, None      # 200 x 300 view: pitch 960 > 900, last windows shifted back
    if name == 'small':
        return synth_u8(100, 6).to(DEV), 128, 0, 2, 1.0, None            # zero fill
    if name == 'rgba':
        return synth_u8(256, 9, alpha=True).to(DEV), 128, 0, 3, 1.0, None
    raise KeyError(name)


@pytest.mark.parametrize('half', [False, True], ids=['fp32', 'half'])
@pytest.mark.parametrize('name', ['tail_chunk', 'overlap_grid', 'crop_view', 'small', 'rgba'])
def test_whole_slide_from_8_bit_equals_the_float_recipe(name, half, monkeypatch):
    import evaluation
    m, dep = _model(half)
    slide, tile, overlap, bs, scale, grid_min = slide_case(name)
    if grid_min is not None:
        monkeypatch.setenv('HDY_NMS_GRID_MIN', str(grid_min))
    if name == 'crop_view':
        assert slide.shape == (200, 300, 3) and slide.stride(0) == 960 and not slide.is_contiguous()
    want = expected(dep, m.headers['det'], slide, tile, overlap, bs, scale)
    nplans = len(m._eng().plans)
    grid_calls, grid = [], ops._nms_grid_launch
    monkeypatch.setattr(ops, '_nms_grid_launch', lambda *a, **k: grid_calls.append(1) or grid(*a, **k))
    got = evaluation.inference_on_slide(dep, slide, tile=tile, overlap=overlap, batch_size=bs, scale=scale)
    assert list(got) == ['det']
    assert_same(got['det'], want, f'{name} half={half}')
    assert len(m._eng().plans) == nplans, 'the 8-bit path built plans of its own: it must run the plans of the float batches'
    if grid_min is not None:
        assert grid_calls, 'the merge did not reach the multi-workgroup NMS'


def test_blank_tiles_are_skipped(monkeypatch):
    import evaluation
    m, dep = _model(True)
    slide = synth_u8(448, 9)
    slide[:, 224:] = 255                                                  # the right half is glass
    slide = slide.to(DEV)
    tile, overlap, bs = 128, 64, 12
    table = np.asarray(evaluation.slide_rois(448, 448, tile, overlap), dtype=np.int32)
    counts = np.asarray(tissue_ref(slide.cpu().numpy(), table.tolist(), tile, tile, 220))
    kept = table[counts >= 0.05 * tile * tile]                            # the rule, restated
    assert 0 < len(kept) < len(table) and any(x0 < 224 < x0 + tile for x0, _ in kept) and not any(x0 >= 224 for x0, _ in kept)
    ran = {'tiles': 0, 'tissue': 0}
    rec, tissue = ops.rec_slide_tiles, ops.slide_tissue

    def spy_rec(slide, origins, first, count, out, pad=2):
        ran['tiles'] += count
        return rec(slide, origins, first, count, out, pad=pad)

    def spy_tissue(*a, **k):
        ran['tissue'] += 1
        return tissue(*a, **k)

    monkeypatch.setattr(ops, 'rec_slide_tiles', spy_rec)
    monkeypatch.setattr(ops, 'slide_tissue', spy_tissue)
    want = expected(dep, m.headers['det'], slide, tile, overlap, bs, origins=kept.tolist())
    got = evaluation.inference_on_slide(dep, slide, tile=tile, overlap=overlap, batch_size=bs, min_tissue=0.05)
    assert_same(got['det'], want, 'skipping')
    assert ran == {'tiles': len(kept), 'tissue': 1}
    ran.update(tiles=0, tissue=0)
    _lib.dispatch_log(reset=True)
    full = evaluation.inference_on_slide(dep, slide, tile=tile, overlap=overlap, batch_size=bs, min_tissue=0.0)
    assert ran == {'tiles': len(table), 'tissue': 0} and 'slide_tissue_u8' not in _lib.dispatch_log()
    assert_same(full['det'], expected(dep, m.headers['det'], slide, tile, overlap, bs), 'no skipping')
    with pytest.raises(ValueError, match='8-bit'):
        evaluation.inference_on_slide(dep, synth.synth_images(1, 128, seed=1)[0].to(DEV), tile=128, min_tissue=0.1)


def test_multi_label_keeps_the_python_merge_on_gathered_tiles():
    import evaluation
    m, dep = _model(True, multi_label=True)
    slide = synth_u8(256, 9).to(DEV)
    want = expected(dep, m.headers['det'], slide, 128, 0, 3)
    got = evaluation.inference_on_slide(dep, slide, tile=128, overlap=0, batch_size=3)['det']
    assert got['labels'].dim() == 2 and got['scores'].dim() == 2
    assert_same(got, want, 'multi_label')
    m.train()
    with pytest.raises(RuntimeError, match='eval-only'):
        m.forward_tiles(slide, ops.slide_origins([(0, 0)], DEV), 0, 1, (128, 128))
    m.eval()


def test_masks_keep_the_python_merge_on_gathered_tiles():
    import evaluation
    from metayolo.models.yolo import Deploy, Model
    cfg = synth.make_cfg('n', 2)
    cfg['headers'][0][3][3] = 1                                           # the mask model of tests/test_gpu_mask.py
    m = Model(cfg, synth.make_hyp(conf_thres=0.05))
    assert not m.load_state_dict(synth.mask_state_dict(m), strict=False).unexpected_keys
    m = m.to(DEV).eval()
    dep = Deploy(m)
    slide = synth_u8(256, 7).to(DEV)
    want = expected(dep, m.headers['det'], slide, 128, 0, 3, compute_masks=True)
    got = evaluation.inference_on_slide(dep, slide, tile=128, overlap=0, batch_size=3, compute_masks=True)['det']
    assert 'masks' in got and got['masks'].shape[1:] == (1, 28, 28)
    assert_same(got, want, 'masks')


def test_whole_slide_repeats_are_bit_identical(monkeypatch):
    import evaluation
    monkeypatch.setenv('HDY_NMS_GRID_MIN', '256')
    m, dep = _model(True)
    slide = synth_u8(448, 9).to(DEV)
    first = evaluation.inference_on_slide(dep, slide, tile=128, overlap=64, batch_size=12)['det']
    assert len(first['boxes']) > 0
    for _ in range(5):
        again = evaluation.inference_on_slide(dep, slide, tile=128, overlap=64, batch_size=12)['det']
        for k, v in first.items():
            assert torch.equal(again[k], v), k
