"""Mask scoring on the MI355X (csrc/mask_score.hip: hdy_label_overlap, hdy_mask_ap_match; ops.label_overlap, ops.mask_ap_match,
DeviceAPMeter.add_batch_masks, evaluation.score_slide_masks): exact equality with the numpy restatement (tests/mask_score_ref.py, itself tied
to the host APMeter and the reference's results by tests/test_mask_score_host.py) on the overlap as sorted triples plus both area arrays, on the
matching, and on the two callers.  Everything is integer counts or one fp32 division of them, so every comparison is exact.  No test provokes a
fault: invalid calls are answered by status on the host (tests/test_mask_score_host.py), and the full-table case is a reported status."""
import os

import numpy as np
import pytest
import torch

import mask_score_ref as ref
from hd_yolo_amd import _lib, ops
from metayolo.models.metrics import APMeter, DeviceAPMeter

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
IOUV10 = np.linspace(0.5, 0.95, 10).astype(np.float32)
NAMES = ('hit', 'live', 'match', 'match_iou')
G = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'mask_ap.npz'), allow_pickle=False)


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def device_overlap(pm, tm, n_pred, n_true, pbase=None, tbase=None, **kw):
    seg = None if pbase is None else (to_dev(np.asarray(pbase, np.int32)), to_dev(np.asarray(tbase, np.int32)))
    pairs, pa, ta = ops.label_overlap(to_dev(pm), to_dev(tm), n_pred, n_true, seg=seg, **kw)
    assert pairs.dtype == torch.int64 and pa.dtype == ta.dtype == torch.int32
    return pairs.cpu().numpy(), pa.cpu().numpy(), ta.cpu().numpy()


def check_overlap(pm, tm, n_pred, n_true, pbase=None, tbase=None, what='', **kw):
    got = device_overlap(pm, tm, n_pred, n_true, pbase, tbase, **kw)
    want = ref.overlap(pm, tm, n_pred, n_true, pbase, tbase)
    for g, w, name in zip(got, want, ('pairs', 'pred_area', 'true_area')):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        np.testing.assert_array_equal(g, w, err_msg=f'{what} {name}')
    return want


def assert_bit_equal(got, want, what=''):
    for g, w, name in zip(got, want, NAMES):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        if g.dtype == np.float32:
            g, w = g.view(np.uint32), w.view(np.uint32)
        np.testing.assert_array_equal(g, w, err_msg=f'{what} {name}')


def device_match(pairs, pa, ta, ps, pl, tl, iouv=IOUV10, prow=None, trow=None, **kw):
    out = ops.mask_ap_match(to_dev(pairs), to_dev(pa), to_dev(ta), to_dev(np.asarray(ps, np.float32)), to_dev(np.asarray(pl, np.int64)),
                            to_dev(np.asarray(tl, np.int64)), iouv, pred_row=None if prow is None else to_dev(np.asarray(prow, np.int32)),
                            true_row=None if trow is None else to_dev(np.asarray(trow, np.int32)), **kw)
    hit, live, match, miou = (t.cpu().numpy() for t in out)
    return hit.view(np.uint16), live, match, miou


def check_match(pairs, pa, ta, ps, pl, tl, what='', **kw):
    got = device_match(pairs, pa, ta, ps, pl, tl, **kw)
    want = ref.match(pairs, pa, ta, ps, pl, tl, IOUV10, **kw)
    assert_bit_equal(got, want, what)
    return got


def relabel(label_map, new_of_old):
    """the map with row r renamed new_of_old[r] (background stays -1; a map without rows is all background)"""
    if not len(new_of_old):
        return np.full(label_map.shape, -1, np.int32)
    return np.where(label_map >= 0, np.asarray(new_of_old)[label_map.clip(0)], -1).astype(np.int32)


def ellipse_case(seed, shape, n_true):
    rng = np.random.default_rng(seed)
    pm, tm, n_pred, source = ref.ellipse_pair(rng, shape, n_true)
    ps, pl, tl = ref.labels_and_scores(rng, n_pred, n_true, source)
    return pm, tm, n_pred, ps, pl, tl


# (name, pred map, truth map, n_pred, n_true, scores, pred labels, truth labels): made once, shared by the overlap and the match tests
def _cases():
    out = {}
    pm, tm, n_pred, ps, pl, tl = ellipse_case(1, (96, 96), 40)
    out['ellipses_96'] = (pm, tm, n_pred, 40, ps, pl, tl)
    pm, tm, n_pred, ps, pl, tl = ellipse_case(2, (37, 61), 12)                     # odd sides: runs wrap row ends, the last wave row is partial
    out['odd_37x61'] = (pm, tm, n_pred, 12, ps, pl, tl)
    rng = np.random.default_rng(3)
    out['background'] = (np.full((40, 50), -1, np.int32), np.full((40, 50), -1, np.int32), 5, 4, rng.uniform(0, 1, 5).astype(np.float32),
                         np.ones(5, np.int64), np.ones(4, np.int64))
    # one prediction over a 128 x 128 map of 300 truths (Voronoi cells of 300 seeds): one hot prediction row, 300 keys that share its high half
    yy, xx = np.mgrid[0:128, 0:128]
    seeds = rng.uniform(0, 128, (300, 2))
    cells = np.argmin((yy[..., None] - seeds[:, 0]) ** 2 + (xx[..., None] - seeds[:, 1]) ** 2, -1).astype(np.int32)
    out['one_over_300'] = (np.zeros((128, 128), np.int32), cells, 1, 300, np.array([0.9], np.float32), np.ones(1, np.int64), np.ones(300, np.int64))
    # a one-pixel checkerboard of four labels on each side, the two boards shifted against each other: no run is longer than one entry
    board = ((yy[:64, :64] % 2) * 2 + xx[:64, :64] % 2).astype(np.int32)
    other = (((yy[:64, :64] // 2) % 2) * 2 + (xx[:64, :64] + yy[:64, :64]) % 2).astype(np.int32)
    out['checkerboard'] = (board, other, 4, 4, np.array([0.4, 0.3, 0.2, 0.1], np.float32), np.array([1, 2, 1, 2]), np.array([1, 2, 2, 1]))
    return out


CASES = _cases()


# ------------------------------------------------------------------------------------------------ 1. the overlap
@pytest.mark.parametrize('name', list(CASES))
def test_overlap_equals_restatement(name):
    pm, tm, n_pred, n_true = CASES[name][:4]
    pairs, pa, ta = check_overlap(pm, tm, n_pred, n_true, what=name)
    if name == 'background':
        assert len(pairs) == 0 and not pa.any() and not ta.any()
    if name == 'one_over_300':
        assert len(pairs) == 300 and pa.tolist() == [128 * 128]
    if name == 'checkerboard':
        assert len(pairs) == 8 and (pairs[:, 2] == 512).all()             # every label meets two of the other side's, on 512 pixels each


def test_overlap_labels_outside_the_rows_are_background():
    rng = np.random.default_rng(4)
    pm = rng.choice(np.array([-7, -1, 0, 1, 2, 3, 65535, 1 << 30], np.int32), (50, 70))      # n_pred = 3: 3, 65535 and 2^30 are background
    tm = rng.choice(np.array([-7, -1, 0, 1, 4, 5, 65535, -(1 << 31)], np.int32), (50, 70))    # n_true = 5: 5 and 65535 are background
    pairs, pa, ta = check_overlap(pm, tm, 3, 5, what='background labels')
    assert set(pairs[:, 0]) == {0, 1, 2} and set(pairs[:, 1]) == {0, 1, 4}
    # the tile bank's 16-bit instance map needs no rewrite: 0xFFFF is not a row
    t16 = np.where(tm < 0, 0xFFFF, tm & 0xFFFF).astype(np.uint16)
    got = ops.label_overlap(to_dev(pm), torch.from_numpy(t16.view(np.int16)).to(DEV), 3, 5)
    want = ref.overlap(pm, t16.astype(np.int32), 3, 5)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g.cpu().numpy(), w)


def test_overlap_segments_with_bases():
    rng = np.random.default_rng(5)
    maps = [ref.ellipse_pair(rng, (48, 48), n)[:3] for n in (9, 1, 14)]
    pm, tm = np.stack([m[0] for m in maps]), np.stack([m[1] for m in maps])
    n_preds, n_trues = [m[2] for m in maps], [9, 1, 14]
    pbase, tbase = np.concatenate(([0], np.cumsum(n_preds)))[:-1], np.concatenate(([0], np.cumsum(n_trues)))[:-1]
    pairs, pa, ta = check_overlap(pm, tm, sum(n_preds), sum(n_trues), pbase, tbase, what='segments')
    # the same thing image by image
    for i in range(3):
        p1, a1, t1 = ref.overlap(pm[i], tm[i], n_preds[i], n_trues[i])
        sel = (pairs[:, 0] >= pbase[i]) & (pairs[:, 0] < pbase[i] + n_preds[i])
        np.testing.assert_array_equal(pairs[sel] - [pbase[i], tbase[i], 0], p1)
        np.testing.assert_array_equal(pa[pbase[i]:pbase[i] + n_preds[i]], a1)


def test_overlap_full_table_is_reported_not_written_past():
    """slots = 8 for about 60 pairs: status[1] counts the failed inserts, the eight slots hold eight true pairs with their exact counts, the areas are still exact, and the wrapper raises"""
    pm, tm, n_pred, n_true = CASES['ellipses_96'][:4]
    want_pairs, want_pa, want_ta = ref.overlap(pm, tm, n_pred, n_true)
    assert len(want_pairs) > 40
    with pytest.raises(_lib.HdyError, match='full'):
        ops.label_overlap(to_dev(pm), to_dev(tm), n_pred, n_true, max_pairs=4)
    slots = 8
    guard = 64                                                                    # int64 words of 0xA5 behind the table
    buf = torch.full((slots * 3 // 2 + guard,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device=DEV)          # = 0xA5 in every byte
    pa = torch.full((n_pred,), 12345, dtype=torch.int32, device=DEV)
    ta = torch.full((n_true,), 12345, dtype=torch.int32, device=DEV)
    status = torch.full((2,), 777, dtype=torch.int32, device=DEV)
    dpm, dtm = to_dev(pm), to_dev(tm)
    _lib.call('hdy_label_overlap', dpm.data_ptr(), dtm.data_ptr(), dpm.numel(), 0, 0, None, None, n_pred, n_true, pa.data_ptr(), ta.data_ptr(),
              buf.data_ptr(), slots * 12, slots, status.data_ptr(), ops.stream_ptr())
    stored, overflow = status.tolist()
    assert stored == slots and overflow > 0
    assert (buf[slots * 3 // 2:].cpu().numpy().view(np.uint8) == 0xA5).all()
    keys, counts = buf[:slots].cpu().numpy(), buf[slots:slots * 3 // 2].cpu().numpy().view(np.int32)
    known = {(int(p), int(t)): int(c) for p, t, c in want_pairs}
    assert len(set(keys.tolist())) == slots
    for k, c in zip(keys.tolist(), counts.tolist()):
        assert c == known[(k >> 32, k & 0xFFFFFFFF)]                              # a stored pair received every one of its adds
    np.testing.assert_array_equal(pa.cpu().numpy(), want_pa)
    np.testing.assert_array_equal(ta.cpu().numpy(), want_ta)


def test_overlap_initialises_its_outputs_and_repeats_identically():
    """a table, areas and status pre-filled with 0xA5 / 12345: the entry point initialises them itself; two runs give the same set"""
    pm, tm, n_pred, n_true = CASES['ellipses_96'][:4]
    want_pairs, want_pa, want_ta = ref.overlap(pm, tm, n_pred, n_true)
    dpm, dtm = to_dev(pm), to_dev(tm)
    slots = 256
    seen = []
    for fill in (-0x5A5A5A5A5A5A5A5B, 0):
        buf = torch.full((slots * 3 // 2,), fill, dtype=torch.int64, device=DEV)
        pa = torch.full((n_pred,), 12345, dtype=torch.int32, device=DEV)
        ta = torch.full((n_true,), 12345, dtype=torch.int32, device=DEV)
        status = torch.full((2,), 777, dtype=torch.int32, device=DEV)
        _lib.call('hdy_label_overlap', dpm.data_ptr(), dtm.data_ptr(), dpm.numel(), 0, 0, None, None, n_pred, n_true, pa.data_ptr(), ta.data_ptr(),
                  buf.data_ptr(), slots * 12, slots, status.data_ptr(), ops.stream_ptr())
        assert status.tolist() == [len(want_pairs), 0]
        keys, counts = buf[:slots].cpu().numpy(), buf[slots:].cpu().numpy().view(np.int32)
        used = keys != -1
        assert (counts[~used] == 0).all()
        order = np.argsort(keys[used])
        got = np.stack([keys[used][order] >> 32, keys[used][order] & 0xFFFFFFFF, counts[used][order]], 1)
        np.testing.assert_array_equal(got, want_pairs)
        np.testing.assert_array_equal(pa.cpu().numpy(), want_pa)
        np.testing.assert_array_equal(ta.cpu().numpy(), want_ta)
        seen.append(got)
    a = ops.label_overlap(dpm, dtm, n_pred, n_true)
    b = ops.label_overlap(dpm, dtm, n_pred, n_true)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    np.testing.assert_array_equal(a[0].cpu().numpy(), seen[0])


def test_overlap_segments_shorter_than_a_wave_step():
    """7 segments of 10 x 10 entries: a step of 4 x 64 entries spans several segments, runs cross their boundaries"""
    rng = np.random.default_rng(9)
    pm, tm = rng.integers(-1, 3, (7, 10, 10)).astype(np.int32), rng.integers(-1, 2, (7, 10, 10)).astype(np.int32)
    pm[2], tm[2] = 0, 0                                                            # whole segments of one label on both sides: the same local row,
    pm[3], tm[3] = 0, 0                                                            # different global rows, back to back
    pbase, tbase = np.arange(7) * 3, np.arange(7) * 2
    pairs, pa, ta = check_overlap(pm, tm, 21, 14, pbase, tbase, what='short segments')
    assert [6, 4, 100] in pairs.tolist() and [9, 6, 100] in pairs.tolist()


def test_wrappers_refuse_what_they_cannot_score():
    z16 = torch.zeros((4, 4), dtype=torch.int16, device=DEV)
    z32 = torch.zeros((4, 4), dtype=torch.int32, device=DEV)
    with pytest.raises(_lib.HdyError, match='label_overlap: a 16-bit true_map'):
        ops.label_overlap(z32, z16, 1, 65536)                                      # 0xFFFF would be a row
    assert len(ops.label_overlap(z32, z16, 1, 65535)[0]) == 1
    with pytest.raises(_lib.HdyError, match='label_overlap: pred_base must be int32'):
        ops.label_overlap(z32[None], z32[None], 1, 1, seg=(torch.zeros(1, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)))
    with pytest.raises(_lib.HdyError, match='mask_ap_match: pred_area must be int32'):
        ops.mask_ap_match(torch.zeros((0, 3), dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV),
                          torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, device=DEV), torch.ones(1, dtype=torch.int64, device=DEV),
                          torch.ones(1, dtype=torch.int64, device=DEV), IOUV10)
    with pytest.raises(_lib.HdyError, match='label_overlap: pred_map must be int32'):
        ops.label_overlap(z32.float(), z32, 1, 1)


# ------------------------------------------------------------------------------------------------ 2. the matching
@pytest.mark.parametrize('name', list(CASES))
def test_match_equals_restatement(name):
    pm, tm, n_pred, n_true, ps, pl, tl = CASES[name]
    pairs, pa, ta = ref.overlap(pm, tm, n_pred, n_true)
    got = check_match(pairs, pa, ta, ps, pl, tl, what=name)
    if name == 'ellipses_96':
        assert (got[2] >= 0).sum() > 10 and (got[1] == 0).sum() > 0               # matches, and predictions that left the curves
    # from the device's own overlap, end to end
    dp, dpa, dta = ops.label_overlap(to_dev(pm), to_dev(tm), n_pred, n_true)
    out = ops.mask_ap_match(dp, dpa, dta, to_dev(ps), to_dev(np.asarray(pl, np.int64)), to_dev(np.asarray(tl, np.int64)), IOUV10)
    assert_bit_equal((out[0].cpu().numpy().view(np.uint16),) + tuple(t.cpu().numpy() for t in out[1:]), got, name + ' end to end')


def test_match_tie_rules_ignored_labels_and_disagreement():
    # two truths with equal IoU (4 / 8) for one prediction: the lowest truth row, or the lowest true_row
    pairs, pa, ta = np.array([[0, 0, 4], [0, 1, 4]]), np.array([8], np.int32), np.array([4, 4], np.int32)
    got = check_match(pairs, pa, ta, [0.9], [1], [1, 1], what='iou tie')
    assert got[2].tolist() == [0] and got[3].tolist() == [0.5] and got[0].tolist() == [1]
    assert check_match(pairs, pa, ta, [0.9], [1], [1, 1], what='iou tie, rows', trow=[5, 2])[2].tolist() == [1]
    # two predictions with equal scores on one truth: the lower prediction row, or the lower pred_row; the IoU plays no part
    pairs, pa, ta = np.array([[0, 0, 3], [1, 0, 6]]), np.array([3, 6], np.int32), np.array([9], np.int32)
    assert check_match(pairs, pa, ta, [0.5, 0.5], [1, 1], [1], what='score tie', pair_iou=0.3)[2].tolist() == [0, -1]
    assert check_match(pairs, pa, ta, [0.5, 0.5], [1, 1], [1], what='score tie, rows', pair_iou=0.3, prow=[3, 1])[2].tolist() == [-1, 0]
    # an ignored truth label and an ignored prediction label only touch (live = 0); a label disagreement stays live and unmatched
    pairs, pa, ta = np.array([[0, 0, 4], [1, 1, 4], [2, 2, 4], [3, 3, 4]]), np.full(4, 4, np.int32), np.full(4, 4, np.int32)
    got = check_match(pairs, pa, ta, [0.9, 0.8, 0.7, 0.6], [1, -1, 2, 3], [-1, 1, 1, 3], what='ignored')
    assert got[1].tolist() == [0, 0, 1, 1] and got[2].tolist() == [-1, -1, -1, 3] and got[0].tolist() == [0, 0, 0, 0x3FF]
    # no predictions, no truths, no pairs
    empty = np.zeros((0, 3), np.int64)
    assert check_match(empty, np.zeros(0, np.int32), np.zeros(3, np.int32), [], [], [1, 1, 1], what='no predictions')[0].shape == (0,)
    assert check_match(empty, np.full(2, 5, np.int32), np.zeros(0, np.int32), [0.5, 0.4], [1, 1], [], what='no truths')[2].tolist() == [-1, -1]


def test_match_permuted_inputs_give_permuted_results():
    pm, tm, n_pred, n_true, ps, pl, tl = CASES['ellipses_96']
    ps = ps.copy()
    ps[::3] = ps[0]                                                                # score ties, so that the rows matter
    pairs, pa, ta = ref.overlap(pm, tm, n_pred, n_true)
    base = check_match(pairs, pa, ta, ps, pl, tl, what='base')
    rng = np.random.default_rng(6)
    op, ot = rng.permutation(n_pred), rng.permutation(n_true)                      # new position -> original row
    inv_p, inv_t = np.argsort(op), np.argsort(ot)
    pm2, tm2 = relabel(pm, inv_p), relabel(tm, inv_t)
    pairs2, pa2, ta2 = ref.overlap(pm2, tm2, n_pred, n_true)
    got = check_match(pairs2, pa2, ta2, ps[op], pl[op], tl[ot], what='permuted', prow=op, trow=ot)
    np.testing.assert_array_equal(got[0], base[0][op])
    np.testing.assert_array_equal(got[1], base[1][op])
    np.testing.assert_array_equal(got[3].view(np.uint32), base[3][op].view(np.uint32))
    np.testing.assert_array_equal(np.where(got[2] >= 0, ot[got[2].clip(0)], -1), base[2][op])


# ------------------------------------------------------------------------------------------------ 3. the meter and the slide
def golden_images():
    return [dict(pred_map=G[f'pred_map_{i}'].astype(np.int32), true_map=G[f'true_map_{i}'].astype(np.int32), scores=G[f'scores_{i}'],
                 pred_labels=G[f'pred_labels_{i}'], true_labels=G[f'true_labels_{i}']) for i in range(int(G['n_images']))]


def meter_inputs(im):
    """one image as add_batch_masks takes it (rows in descending score order, masks and boxes that paste back into the label map) and as the
    host APMeter takes it (dense masks of the same label maps)"""
    order = np.argsort(-im['scores'], kind='stable')
    inv = np.argsort(order)
    pm = relabel(im['pred_map'], inv)
    n, m = len(order), len(im['true_labels'])
    masks, boxes = ref.paste_inputs(pm, n)
    out = {'boxes': to_dev(boxes), 'scores': to_dev(im['scores'][order]), 'labels': to_dev(im['pred_labels'][order]), 'masks': to_dev(masks)}
    tgt = {'labels': to_dev(im['true_labels']), 'instances': to_dev(im['true_map'])}
    host_out = {'scores': torch.from_numpy(im['scores'][order]), 'labels': torch.from_numpy(im['pred_labels'][order]),
                'masks': torch.from_numpy(ref.dense_masks(pm, n))}
    host_tgt = {'labels': torch.from_numpy(im['true_labels']), 'masks': torch.from_numpy(ref.dense_masks(im['true_map'], m))}
    return out, tgt, host_out, host_tgt, pm


def assert_stats_equal(st, want):
    assert [int(v) for v in st['labels']] == [int(v) for v in want['labels']] and [int(v) for v in st['counts']] == [int(v) for v in want['counts']]
    for k in ('ap', 'p', 'r', 'f1', 'py'):
        np.testing.assert_array_equal(st[k], want[k], err_msg=k)


def test_add_batch_masks_equals_host_apmeter_and_reproduces_the_golden():
    rng = np.random.default_rng(7)
    images = golden_images()
    for n_true in (16, 1, 22):                                                      # 6 images of 64 x 64 in two batches of three; one has no prediction
        pm, tm, n_pred, source = ref.ellipse_pair(rng, (64, 64), n_true)
        ps, pl, tl = ref.labels_and_scores(rng, n_pred, n_true, source)
        images.append(dict(pred_map=pm, true_map=tm, scores=ps, pred_labels=pl, true_labels=tl))
    host, dev, gold = APMeter(), DeviceAPMeter(), DeviceAPMeter()
    for b in range(2):
        outs, tgts = [], []
        for im in images[3 * b:3 * b + 3]:
            o, t, ho, ht, pm = meter_inputs(im)
            # the paste gives the label map back, so the two meters see the same masks
            assert torch.equal(ops.paste_label_map(o['masks'], o['boxes'], (64, 64)).cpu(), torch.from_numpy(pm))
            outs.append(o)
            tgts.append(t)
            host.add(ho, ht, iou_type='masks')
        if b == 1:                                                                   # the tile bank's 16-bit form for one batch
            for t in tgts:
                t['instances'] = torch.from_numpy(np.where(t['instances'].cpu().numpy() < 0, 0xFFFF, t['instances'].cpu().numpy()).astype(np.uint16).view(np.int16)).to(DEV)
        dev.add_batch_masks(outs, tgts, (64, 64))
        if b == 0:
            gold.add_batch_masks(outs, tgts, (64, 64))
    with pytest.raises(_lib.HdyError, match='full'):                                 # max_pairs reaches the overlap: too small a table is reported,
        DeviceAPMeter().add_batch_masks(outs, tgts, (64, 64), max_pairs=4)
    roomy = DeviceAPMeter()                                                          # a larger one changes nothing
    roomy.add_batch_masks(outs, tgts, (64, 64), max_pairs=4096)
    assert torch.equal(roomy._batches[0][2], dev._batches[1][2]) and torch.equal(roomy._batches[0][3], dev._batches[1][3])
    want = host.ap_per_class(iouv=torch.linspace(0.5, 0.95, 10), ignore=[-100, -1])
    assert dev.n_pred == host.n_pred and dev.n_true == host.n_true
    np.testing.assert_array_equal(dev.scores, host.scores)
    np.testing.assert_array_equal(dev.y_pred, host.y_pred)
    np.testing.assert_array_equal(dev.y_true, host.y_true)
    assert_stats_equal(dev.ap_per_class(), want)
    # the reference's own AP on the golden's three images
    st = gold.ap_per_class()
    assert np.array_equal(np.array(st['labels']), G['labels']) and np.array_equal(np.array(st['counts']), G['counts'])
    for k in ('ap', 'p', 'r', 'f1', 'py'):
        np.testing.assert_array_equal(np.asarray(st[k], np.float64), G[k], err_msg=k)


def test_score_slide_masks_equals_the_meter_fed_the_same_maps():
    import evaluation
    rng = np.random.default_rng(8)
    n_true = 220
    pm, tm, n_pred, source = ref.ellipse_pair(rng, (512, 512), n_true, r=(5.0, 12.0))
    ps, pl, tl = ref.labels_and_scores(rng, n_pred, n_true, source)
    order = np.argsort(-ps, kind='stable')                                          # rows in descending score order, as a slide result has them
    inv = np.argsort(order)
    pm, ps, pl = relabel(pm, inv), ps[order], pl[order]
    st = evaluation.score_slide_masks({'label_map': to_dev(pm), 'scores': to_dev(ps), 'labels': to_dev(pl)}, {'label_map': to_dev(tm), 'labels': to_dev(tl)})
    pairs, pa, ta = ref.overlap(pm, tm, n_pred, n_true)
    np.testing.assert_array_equal(st['pairs'].cpu().numpy(), pairs)
    np.testing.assert_array_equal(st['pred_area'].cpu().numpy(), pa)
    np.testing.assert_array_equal(st['true_area'].cpu().numpy(), ta)
    want = ref.match(pairs, pa, ta, ps, pl, tl, IOUV10)
    assert_bit_equal((st['hit'].cpu().numpy().view(np.uint16), st['live'].cpu().numpy(), st['match'].cpu().numpy(), st['match_iou'].cpu().numpy()), want, 'slide')
    assert (want[2] >= 0).sum() > 100
    # the meter, fed the same maps as one image (instances of up to 27 pixels a side fit the 28 x 28 mask of paste_inputs)
    masks, boxes = ref.paste_inputs(pm, n_pred)
    meter = DeviceAPMeter()
    meter.add_batch_masks([{'boxes': to_dev(boxes), 'scores': to_dev(ps), 'labels': to_dev(pl), 'masks': to_dev(masks)}],
                          [{'labels': to_dev(tl), 'instances': to_dev(tm)}], (512, 512))
    assert_stats_equal(st, meter.ap_per_class())


def test_evaluation_cli_prints_the_mask_score(capsys, monkeypatch):
    """python evaluation.py --slide S --u8 --masks --label-map --score: the box score line is followed by the mask score line, whose figures are
    those of score_slide_masks on the same synthetic sets"""
    import re
    import sys
    import evaluation
    from hd_yolo_amd import synth
    monkeypatch.setattr(sys, 'argv', ['evaluation.py', '--variant', 'n', '--nc', '2', '--imgsz', '128', '--batch-size', '2', '--batches', '1',
                                      '--slide', '256', '--u8', '--masks', '--label-map', '--score'])
    evaluation.main()
    out = capsys.readouterr().out
    assert re.search(r'^score: \d+ detections x \d+ truths, mAP@\.5 ', out, flags=re.M)
    m = re.search(r'^mask score: (\d+) detections x (\d+) truths on a 256 x 256 label map, (\d+) overlapping pairs, mask mAP@\.5 ([0-9.]+) in ', out, flags=re.M)
    assert m, out
    tb, tl, pb, ps, pl = synth.synth_slide_truth(max(1, int((256 / 40.0) ** 2)), 256, 2, seed=5)
    assert (int(m.group(1)), int(m.group(2))) == (len(ps), len(tl)) and int(m.group(3)) > 0
    # the same figure from the restatement: one fixed disc pasted into every box, detections in descending score order
    yy, xx = np.mgrid[0:28, 0:28]
    disc = (((yy - 13.5) ** 2 + (xx - 13.5) ** 2) <= 13.5 ** 2).astype(np.float32)
    order = np.argsort(-ps, kind='stable')
    pm = ops.paste_label_map(to_dev(np.broadcast_to(disc, (len(ps), 28, 28))), to_dev(pb[order]), (256, 256)).cpu().numpy()
    tm = ops.paste_label_map(to_dev(np.broadcast_to(disc, (len(tl), 28, 28))), to_dev(tb), (256, 256)).cpu().numpy()
    meter = ref.RefMeter()
    meter.add(pm, ps[order], pl[order], tm, tl)
    assert f'{float(meter.ap_per_class()["ap"][:, 0].mean()):.4f}' == m.group(4)
    assert int(m.group(3)) == len(ref.overlap(pm, tm, len(ps), len(tl))[0])
