"""Segmentation summaries on the host (metayolo.models.metrics.segmentation_counts / segmentation_ratios: PQ, per-class PQ, AJI, Dice from
the sparse overlap of two label maps) against the brute-force restatement tests/seg_summary_ref.py, hand-computed cases, pooling, and the
host logic of the validation loader metayolo.datasets.BankTiles.  No GPU and no HIP library: everything here is torch on the CPU.

Tolerances: every integer field is compared exactly.  iou_sum is a float64 sum of at most 10^6 terms in (0.5, 1], each a correctly rounded
quotient: whatever the order of the additions the relative error stays below n * 2^-53 < 1.2e-10, so 1e-9 relative."""
import numpy as np
import pytest
import torch

import seg_summary_ref as ref
from hd_yolo_amd import synth
from metayolo.datasets import BankTiles, bank_batches, bank_origins, check_bank_stride
from metayolo.models.metrics import SEG_COUNT_KEYS, segmentation_counts, segmentation_counts_to_host, segmentation_ratios

REL = 1e-9


def torch_counts(pairs, pa, ta, pl=None, tl=None, nc=None):
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a))   # noqa: E731
    out = segmentation_counts(t(pairs), t(pa), t(ta), t(pl), t(tl), nc=nc)
    for k, v in out.items():
        assert v.dtype == (torch.float64 if k.startswith('iou_sum') else torch.int64), (k, v.dtype)
    return segmentation_counts_to_host(out)


def assert_counts_equal(got, want, what=''):
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for k, w in want.items():
        if k.startswith('iou_sum'):
            np.testing.assert_allclose(np.asarray(got[k], np.float64), np.asarray(w, np.float64), rtol=REL, atol=0, err_msg=f'{what} {k}')
        else:
            np.testing.assert_array_equal(np.asarray(got[k]), np.asarray(w), err_msg=f'{what} {k}')


def random_case(seed, shape, n_pred, n_true, extra=(0, 0), nc=3):
    rng = np.random.default_rng(seed)
    pm, rows_p = ref.random_map(rng, shape, n_pred, extra[0])
    tm, rows_t = ref.random_map(rng, shape, n_true, extra[1])
    if n_pred and n_true and seed % 2:                       # some predictions that are their truth: IoU 1, and equal IoUs among the rest
        keep = rng.random(n_true) < 0.4
        pm = np.where((tm >= 0) & keep[tm.clip(0)], tm % n_pred, pm).astype(np.int32)
    pl = rng.integers(1, nc + 1, rows_p).astype(np.int64)
    tl = rng.integers(1, nc + 1, rows_t).astype(np.int64)
    if rows_p:
        pl[rng.integers(0, rows_p)] = -100                    # an ignored label belongs to no class
    return pm, tm, rows_p, rows_t, pl, tl, nc


# (seed, shape, predictions, truths, rows named in the areas but absent from the map)
RANDOM = [(1, (64, 64), 12, 9, (0, 0)), (2, (64, 64), 40, 40, (3, 2)), (3, (96, 128), 25, 40, (0, 5)), (4, (96, 128), 40, 17, (4, 0)),
          (5, (64, 64), 0, 14, (0, 0)), (6, (96, 128), 21, 0, (0, 0)), (7, (64, 64), 0, 0, (0, 0)), (8, (64, 64), 0, 0, (2, 3)),
          (9, (96, 128), 1, 1, (0, 0)), (11, (64, 64), 33, 30, (1, 1))]


@pytest.mark.parametrize('seed,shape,n_pred,n_true,extra', RANDOM)
def test_random_maps_equal_the_brute_force(seed, shape, n_pred, n_true, extra):
    pm, tm, rows_p, rows_t, pl, tl, nc = random_case(seed, shape, n_pred, n_true, extra)
    pairs, pa, ta = ref.overlap(pm, tm, rows_p, rows_t)
    if extra[0] and n_pred:
        assert (pa == 0).any()                                                      # rows without a pixel are no instances
    want = ref.counts(pairs, pa, ta, pl, tl, nc)
    got = torch_counts(pairs, pa, ta, pl, tl, nc)
    assert_counts_equal(got, want, f'seed {seed}')
    for k, w in ref.ratios(want).items():
        assert segmentation_ratios(got)[k] == pytest.approx(w, rel=REL, abs=0), k
    # without labels: the same class-agnostic counts and no per-class ones; nc=None reads the largest label
    plain = torch_counts(pairs, pa, ta)
    assert_counts_equal(plain, {k: want[k] for k in SEG_COUNT_KEYS}, f'seed {seed} unlabelled')
    assert 'mpq' not in segmentation_ratios(plain)
    if rows_p and rows_t:
        top = int(max(pl.max(), tl.max()))
        auto = torch_counts(pairs, pa, ta, pl, tl)
        assert len(auto['tp_c']) == top
        assert_counts_equal(auto, ref.counts(pairs, pa, ta, pl, tl, top), f'seed {seed} nc=None')


def test_random_cases_cover_what_they_claim():
    """the brute-force side: true positives, both kinds of misses and fragments (more pairs than rows on either side) are all present"""
    fragments = False
    total = {'tp': 0, 'fp': 0, 'fn': 0}
    for seed, shape, n_pred, n_true, extra in RANDOM:
        pm, tm, rows_p, rows_t, pl, tl, nc = random_case(seed, shape, n_pred, n_true, extra)
        pairs, pa, ta = ref.overlap(pm, tm, rows_p, rows_t)
        c = ref.counts(pairs, pa, ta)
        for k in total:
            total[k] += c[k]
        fragments |= len(pairs) > max(rows_p, rows_t) > 0
    assert total['tp'] >= 10 and total['fp'] >= 10 and total['fn'] >= 10 and fragments


def _maps(h, w, pred_rects, true_rects):
    """label maps from (row, y0, y1, x0, x1) rectangles painted in order"""
    pm, tm = np.full((h, w), -1, np.int32), np.full((h, w), -1, np.int32)
    for m, rects in ((pm, pred_rects), (tm, true_rects)):
        for r, y0, y1, x0, x1 in rects:
            m[y0:y1, x0:x1] = r
    return pm, tm


def _summary(pm, tm, n_pred, n_true):
    pairs, pa, ta = ref.overlap(pm, tm, n_pred, n_true)
    c = torch_counts(pairs, pa, ta)
    return c, segmentation_ratios(c)


def test_hand_one_perfect_match():
    pm, tm = _maps(8, 8, [(0, 2, 5, 1, 5)], [(0, 2, 5, 1, 5)])
    c, r = _summary(pm, tm, 1, 1)
    assert (c['tp'], c['fp'], c['fn'], c['C'], c['U'], c['inter_sum'], c['pred_sum'], c['true_sum']) == (1, 0, 0, 12, 12, 12, 12, 12)
    assert c['iou_sum'] == 1.0 and r['pq'] == r['sq'] == r['dq'] == r['aji'] == r['dice'] == 1.0


def test_hand_one_prediction_covering_two_truths():
    """prediction 0 = columns 0..9 of a 1 x 12 strip (10 px); truth 0 = columns 0..6 (7 px), truth 1 = columns 7..9 (3 px).
    IoU(0, 0) = 7 / 10 > 0.5: TP; IoU(0, 1) = 3 / 10: truth 1 is a FN.  AJI lets the prediction serve both truths: C = 7 + 3,
    U = (10 + 7 - 7) + (10 + 3 - 3) = 20 — the second truth brings the whole prediction into the union again."""
    pm, tm = _maps(1, 12, [(0, 0, 1, 0, 10)], [(0, 0, 1, 0, 7), (1, 0, 1, 7, 10)])
    c, r = _summary(pm, tm, 1, 2)
    assert (c['tp'], c['fp'], c['fn']) == (1, 0, 1) and c['iou_sum'] == pytest.approx(0.7, rel=REL)
    assert (c['C'], c['U']) == (10, 20) and (c['inter_sum'], c['pred_sum'], c['true_sum']) == (10, 10, 10)
    assert r['dq'] == pytest.approx(1 / 1.5, rel=REL) and r['sq'] == pytest.approx(0.7, rel=REL) and r['pq'] == pytest.approx(0.7 / 1.5, rel=REL)
    assert r['aji'] == 0.5 and r['dice'] == 1.0
    # the other way round: one truth under two predictions.  The unused prediction's area goes to U, the truth is matched once.
    c, r = _summary(tm, pm, 2, 1)
    assert (c['tp'], c['fp'], c['fn']) == (1, 1, 0) and (c['C'], c['U']) == (7, 10 + 3)


def test_hand_exact_aji_tie_goes_to_the_lower_row():
    """IoU = i / (a + b - i) for a truth of a pixels, a prediction of b pixels and i shared ones.  With a = 3: (i = 1, b = 1) gives 1/3 and
    (i = 2, b = 5) gives 2/6, and 1 + 2 = 3 shared pixels fit the truth: two different pairs of equal IoU, told apart by neither float
    nor integer terms alone.  The lower prediction row wins and the other prediction's whole area goes to U."""
    pm, tm = np.full((2, 8), -1, np.int32), np.full((2, 8), -1, np.int32)
    tm[0, 0:3] = 0                                  # truth 0: 3 px
    pm[0, 0:2] = 1                                  # prediction 1 shares 2 px ...
    pm[1, 0:3] = 1                                  # ... and owns 3 more: area 5, union 3 + 5 - 2 = 6 -> IoU 2/6
    pm[0, 2] = 0                                    # prediction 0: 1 px, all shared: union 3 + 1 - 1 = 3 -> IoU 1/3
    pairs, pa, ta = ref.overlap(pm, tm, 2, 1)
    assert pairs.tolist() == [[0, 0, 1], [1, 0, 2]] and pa.tolist() == [1, 5] and ta.tolist() == [3]
    c = torch_counts(pairs, pa, ta)
    assert (c['C'], c['U']) == (1, 3 + 5)           # the lower row wins: C = 1, U = union(0, 0) = 3 plus prediction 1's whole area
    assert (c['tp'], c['fp'], c['fn']) == (0, 2, 1) and c['iou_sum'] == 0.0
    r = segmentation_ratios(c)
    assert r['aji'] == 1 / 8 and r['pq'] == r['sq'] == r['dq'] == 0.0 and r['dice'] == pytest.approx(2 * 3 / (6 + 3), rel=REL)
    # the same tie with the rows exchanged: now the 2/6 pair is the lower row and wins
    pm2 = np.where(pm >= 0, 1 - pm, -1).astype(np.int32)
    c2 = torch_counts(*ref.overlap(pm2, tm, 2, 1))
    assert (c2['C'], c2['U']) == (2, 6 + 1)
    assert_counts_equal(c, {**ref.counts(pairs, pa, ta)}, 'tie')


def test_hand_iou_of_exactly_one_half_is_no_true_positive():
    """prediction 0 = columns 0..2, truth 0 = columns 1..3 of a strip: inter 2, areas 3 and 3, union 4: 3 inter == area_p + area_t"""
    pm, tm = _maps(1, 8, [(0, 0, 1, 0, 3)], [(0, 0, 1, 1, 4)])
    pairs, pa, ta = ref.overlap(pm, tm, 1, 1)
    assert pairs.tolist() == [[0, 0, 2]] and 3 * 2 == int(pa[0]) + int(ta[0])
    c = torch_counts(pairs, pa, ta)
    assert (c['tp'], c['fp'], c['fn']) == (0, 1, 1) and c['iou_sum'] == 0.0
    assert (c['C'], c['U']) == (2, 4)                                               # AJI still pairs them
    # one pixel more of overlap on the same areas is a true positive
    pm, tm = _maps(1, 8, [(0, 0, 1, 0, 3)], [(0, 0, 1, 0, 3)])
    assert torch_counts(*ref.overlap(pm, tm, 1, 1))['tp'] == 1


def test_empty_denominators_are_zero():
    c = torch_counts(np.zeros((0, 3), np.int64), np.zeros(0, np.int32), np.zeros(0, np.int32))
    assert all(c[k] == 0 for k in SEG_COUNT_KEYS)
    assert segmentation_ratios(c) == {'pq': 0.0, 'sq': 0.0, 'dq': 0.0, 'aji': 0.0, 'dice': 0.0}
    from metayolo.models.metrics import DeviceAPMeter
    s = DeviceAPMeter().segmentation_summary()                                      # no add_batch_masks call: the all-zero summary
    assert all(s[k] == 0 for k in SEG_COUNT_KEYS) and all(s[k] == 0.0 for k in ('pq', 'sq', 'dq', 'aji', 'dice'))


def test_counts_pool_by_addition():
    """three map pairs added one by one equal their concatenation with row bases (what a batch is to DeviceAPMeter.add_batch_masks)"""
    parts, cat_pairs, cat_pa, cat_ta, cat_pl, cat_tl = [], [], [], [], [], []
    base_p = base_t = 0
    for seed, shape, n_pred, n_true, extra in (RANDOM[0], RANDOM[2], RANDOM[4]):
        pm, tm, rows_p, rows_t, pl, tl, nc = random_case(seed, shape, n_pred, n_true, extra)
        pairs, pa, ta = ref.overlap(pm, tm, rows_p, rows_t)
        parts.append(torch_counts(pairs, pa, ta, pl, tl, nc))
        cat_pairs.append(pairs + [base_p, base_t, 0])
        cat_pa.append(pa), cat_ta.append(ta), cat_pl.append(pl), cat_tl.append(tl)
        base_p, base_t = base_p + rows_p, base_t + rows_t
    whole = torch_counts(np.concatenate(cat_pairs), np.concatenate(cat_pa), np.concatenate(cat_ta), np.concatenate(cat_pl), np.concatenate(cat_tl), 3)
    summed = {k: sum(np.asarray(p[k]) for p in parts) for k in whole}
    assert_counts_equal(whole, summed, 'pooled')
    assert whole['tp'] > 0 and whole['fn'] > 0


# ------------------------------------------------------------------------------------------------ BankTiles: the host logic
def test_bank_batches_and_origins():
    assert bank_batches(5, 2) == [(0, 2), (2, 2), (4, 1)]
    assert bank_batches(4, 4) == [(0, 4)]
    assert bank_batches(0, 3) == []
    assert bank_origins(3, 128).tolist() == [[0, 0], [0, 128], [0, 256]] and bank_origins(3, 128).dtype == np.int32
    with pytest.raises(ValueError, match='batch_size=0'):
        bank_batches(5, 0)


def test_bank_tiles_on_the_cpu_yields_the_bank():
    bank = synth.synth_tile_bank(5, 32, 3, seed=1, nmin=0, nmax=6, instances=True)
    loader = BankTiles(bank, 2, device='cpu')
    loader.set_epoch(3)
    assert len(loader) == 3 and loader.batches == [(0, 2), (2, 2), (4, 1)] and loader.tile == (32, 32)
    assert loader.slide.shape == (5 * 32, 32, 3) and loader.slide.data_ptr() == bank.d_tiles.data_ptr()
    assert loader.origins.tolist() == [[0, 32 * t] for t in range(5)]
    seen = 0
    for (imgs, targets), (span, targets8) in zip(loader, loader.u8_batches()):
        assert isinstance(imgs, tuple) and len(imgs) == len(targets) == span[1] and span[0] == seen
        for i, (x, tgt, tgt8) in enumerate(zip(imgs, targets, targets8)):
            t = seen + i
            assert x.dtype == torch.float32 and torch.equal(x, torch.from_numpy(bank.tiles[t]).permute(2, 0, 1).float() / 255)
            ann = tgt['anns']['det'][0]
            lo, hi = int(bank.offsets[t]), int(bank.offsets[t + 1])
            assert int(tgt['image_id']) == t and tgt['size'].tolist() == [32, 32]
            assert ann['boxes'].dtype == torch.float32 and np.array_equal(ann['boxes'].numpy(), bank.boxes[lo:hi])
            assert ann['labels'].dtype == torch.int64 and np.array_equal(ann['labels'].numpy(), bank.labels[lo:hi])
            assert ann['instances'].data_ptr() == bank.d_instances[t].data_ptr()                     # a view of the bank's bits
            assert np.array_equal(ann['instances'].numpy().view(np.uint16), bank.instances[t])
            assert tgt8['anns']['det'][0]['boxes'].data_ptr() == ann['boxes'].data_ptr() or hi == lo
        seen += span[1]
    assert seen == 5
    # masks=True on a bank without a map degrades to box-only targets; masks=False leaves the map out
    plain = synth.synth_tile_bank(2, 32, 3, seed=1, nmin=1, nmax=3)
    assert 'instances' not in next(iter(BankTiles(plain, 2, device='cpu')))[1][0]['anns']['det'][0]
    assert 'instances' not in next(iter(BankTiles(bank, 2, device='cpu', masks=False)))[1][0]['anns']['det'][0]


def test_bank_tiles_refusals_name_the_bank_and_the_number(tmp_path):
    bank = synth.synth_tile_bank(2, 48, 3, seed=2, nmin=1, nmax=3)
    check_bank_stride(bank, 16)
    with pytest.raises(ValueError, match=r'tile bank \(2 tiles of 48 x 48\): tile height 48 is not a multiple of the model\'s largest stride 32'):
        check_bank_stride(bank, 32)
    path = str(tmp_path / 'held_out.npz')
    bank.save(path)
    from hd_yolo_amd.augment import TileBank
    loaded = TileBank.load(path)
    with pytest.raises(ValueError, match=r'held_out\.npz: tile height 48 .* stride 32'):
        BankTiles(loaded, 2, device='cpu').check_stride(32)
    # 4-byte pixels that are a view of something wider cannot be read as one slide
    rgba = TileBank(np.zeros((2, 32, 32, 4), np.uint8), np.zeros((0, 4), np.float32), np.zeros(0, np.int64), np.zeros(3, np.int64)).to('cpu')
    BankTiles(rgba, 2, device='cpu')
    rgba.d_tiles = torch.zeros((2, 32, 40, 4), dtype=torch.uint8)[:, :, :32]
    with pytest.raises(ValueError, match=r'tile bank \(2 tiles of 32 x 32\): 4-byte pixels with strides \(5120, 160, 4, 1\)'):
        BankTiles(rgba, 2, device='cpu')
