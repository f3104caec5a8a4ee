"""Validation on a held-out tile bank on the MI355X (metayolo.datasets.BankTiles, val_nuclei.run's 8-bit path and mask scoring,
DeviceAPMeter.segmentation_summary, train.py --val-bank).  Shapes: the smallest that still have a partial batch, three pyramid levels and the
mask path — a bank of 5 tiles of 128 x 128 in batches of 2 (the last of one tile), yolov5n with nc = 3 and synthetic weights, bf16, and
conf_thres = 0.001 so that random weights still yield detections.

Equalities are exact: the 8-bit path gathers the same correctly rounded bytes / 255 into the same plan as the float path, and both scoring
routes run the same kernels on the same rows.  The segmentation summaries are integer counts (exact) and one float64 sum of at most a few
thousand quotients (1e-9 relative, see tests/test_seg_summary_host.py) against the brute force tests/seg_summary_ref.py."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import seg_summary_ref as ref
from hd_yolo_amd import ops, synth
from metayolo.datasets import BankTiles
from metayolo.models.metrics import DeviceAPMeter

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, SIDE, NC, BATCH = 5, 128, 3, 2
REL = 1e-9


def make_bank():
    return synth.synth_tile_bank(N, SIDE, NC, instances=True)


def make_model(masks):
    from metayolo.models.yolo import Model
    cfg = synth.make_cfg('n', NC)
    if masks:
        cfg['headers'][0][3][3] = 1                                   # one shared mask class, as scripts/bench_mask.py builds it
    m = Model(cfg, synth.make_hyp(conf_thres=0.001))
    m.load_state_dict(synth.synth_state_dict(synth.shapes_of(m), seed=0), strict=False)
    return m.to(DEV).eval()


@pytest.fixture(scope='module')
def bank():
    return make_bank()


@pytest.fixture(scope='module')
def loader(bank):
    return BankTiles(bank, BATCH, device=DEV)


@pytest.fixture(scope='module')
def box_model():
    return make_model(False)


@pytest.fixture(scope='module')
def mask_model():
    return make_model(True)


@pytest.fixture(scope='module')
def mask_runs(mask_model, loader):
    """val_nuclei.run of the mask model from the bank and from a plain list of the loader's (imgs, targets) tuples, made once"""
    import val_nuclei
    from_bank = val_nuclei.run(mask_model, loader, half=True, device_metrics=True)
    from_list = val_nuclei.run(mask_model, list(loader), half=True, device_metrics=True)
    return from_bank, from_list


# ------------------------------------------------------------------------------------------------ 1. truth rows
def test_loader_hands_back_the_bank(bank, loader):
    assert len(loader) == 3 and loader.batches == [(0, 2), (2, 2), (4, 1)]
    boxes, labels, counts, t = [], [], [], 0
    for imgs, targets in loader:
        assert isinstance(imgs, tuple) and len(imgs) == len(targets)
        for x, tgt in zip(imgs, targets):
            ann = tgt['anns']['det'][0]
            assert x.device == DEV and x.dtype == torch.float32 and x.shape == (3, SIDE, SIDE)
            assert torch.equal(x.cpu(), torch.from_numpy(bank.tiles[t]).permute(2, 0, 1).float() / 255)
            assert ann['boxes'].dtype == torch.float32 and ann['labels'].dtype == torch.int64 and int(tgt['image_id']) == t
            assert np.array_equal(ann['instances'].cpu().numpy().view(np.uint16), bank.instances[t])
            assert ann['instances'].data_ptr() == bank.d_instances[t].data_ptr()                    # the bank's bits, no copy
            boxes.append(ann['boxes'].cpu().numpy())
            labels.append(ann['labels'].cpu().numpy())
            counts.append(len(ann['labels']))
            t += 1
    assert t == N
    assert np.array_equal(np.concatenate(boxes), bank.boxes) and np.array_equal(np.concatenate(labels), bank.labels)
    assert np.array_equal(np.concatenate(([0], np.cumsum(counts))), bank.offsets)
    assert loader.slide.shape == (N * SIDE, SIDE, 3) and loader.origins.cpu().tolist() == [[0, SIDE * i] for i in range(N)]


# ------------------------------------------------------------------------------------------------ 2. 8-bit path == float path
def test_forward_tiles_equals_the_float_batch(box_model, loader):
    box_model.half()
    detections = 0
    for (imgs, _), ((first, count), _) in zip(loader, loader.u8_batches()):
        _, want = box_model(torch.stack(imgs))
        _, got = box_model.forward_tiles(loader.slide, loader.origins, first, count, loader.tile, compute_masks=False, device_outputs=False)
        assert len(got) == len(want) == count
        for g, w in zip(got, want):
            for k in ('boxes', 'scores', 'labels'):
                assert g['det'][k].dtype == w['det'][k].dtype and torch.equal(g['det'][k], w['det'][k]), (first, k)
            detections += len(g['det']['scores'])
    box_model.float()
    assert detections > 0                                                           # otherwise the comparison is vacuous


# ------------------------------------------------------------------------------------------------ 3. run on the bank == run on a plain loader
def test_run_on_the_bank_equals_run_on_a_plain_loader(box_model, bank, loader):
    import val_nuclei
    fit_bank, stats_bank, _ = val_nuclei.run(box_model, loader, half=True, device_metrics=True)
    fit_list, stats_list, _ = val_nuclei.run(box_model, list(loader), half=True, device_metrics=True)
    assert fit_bank == fit_list and stats_bank == stats_list
    assert set(stats_bank['det']) == {'mp', 'mr', 'f1', 'map50', 'map', 'fitness'}                  # no mask branch: no 'masks'
    with pytest.raises(ValueError, match=r"tile bank \(1 tiles of 48 x 48\): tile height 48 is not a multiple of the model's largest stride 32"):
        val_nuclei.run(box_model, BankTiles(synth.synth_tile_bank(1, 48, NC, nmin=1, nmax=2), 1, device=DEV), device_metrics=True)


# ------------------------------------------------------------------------------------------------ 4. mask summaries against the brute force
def test_segmentation_summary_equals_the_brute_force(bank, loader):
    rng = np.random.default_rng(17)
    meter, parts = DeviceAPMeter(), []
    n_pairs = 0
    for _, targets in loader:
        outs, tgts = [], []
        for tgt in targets:
            ann = tgt['anns']['det'][0]
            t = int(tgt['image_id'])
            n_true = len(ann['labels'])
            rows = np.nonzero(rng.random(n_true) < 0.8)[0]                           # some truths are left without a row
            b = ann['boxes'].cpu().numpy()[rows] + rng.integers(-3, 4, (len(rows), 4)).astype(np.float32)
            b[rng.random(len(rows)) < 0.2] += np.float32(60.0)                       # some rows sit 60 px away from their truth
            scores = np.linspace(0.9, 0.1, len(rows)).astype(np.float32)             # rows in descending score order
            out = {'boxes': torch.from_numpy(b).to(DEV), 'scores': torch.from_numpy(scores).to(DEV), 'labels': ann['labels'][torch.from_numpy(rows).to(DEV)],
                   'masks': torch.ones((len(rows), 1, 28, 28), device=DEV)}
            outs.append(out)
            tgts.append({'labels': ann['labels'], 'instances': ann['instances']})
            pm = ops.paste_label_map(out['masks'], out['boxes'], (SIDE, SIDE)).cpu().numpy()
            tm = np.where(bank.instances[t] == 0xFFFF, -1, bank.instances[t].astype(np.int32))
            pairs, pa, ta = ref.overlap(pm, tm, len(rows), n_true)
            n_pairs += len(pairs)
            parts.append(ref.counts(pairs, pa, ta))
        meter.add_batch_masks(outs, tgts, (SIDE, SIDE))
    want = ref.pool(parts)
    assert want['tp'] >= 1 and want['fp'] >= 1 and want['fn'] >= 1 and n_pairs > want['tp']
    got = meter.segmentation_summary()
    for k in ref.INT_KEYS:
        assert isinstance(got[k], int) and got[k] == want[k], (k, got[k], want[k])
    assert got['iou_sum'] == pytest.approx(want['iou_sum'], rel=REL, abs=0)
    for k, w in ref.ratios(want).items():
        assert got[k] == pytest.approx(w, rel=REL, abs=0), k
    assert got['tp'] + got['fn'] == int(bank.has_mask.sum())
    # the box meter is untouched by the mask route and an unused meter reports zeros
    assert DeviceAPMeter().segmentation_summary()['U'] == 0


# ------------------------------------------------------------------------------------------------ 5. run with masks
def test_run_scores_masks_and_keeps_the_box_metrics(mask_model, bank, loader, mask_runs):
    (fit_bank, stats_bank, _), (fit_list, stats_list, _) = mask_runs
    masks = stats_bank['det']['masks']
    assert set(masks) >= {'mp', 'mr', 'f1', 'map50', 'map', 'fitness', 'pq', 'sq', 'dq', 'aji', 'dice', 'tp', 'fp', 'fn', 'iou_sum', 'C', 'U',
                          'inter_sum', 'pred_sum', 'true_sum'}
    # the predicted instances, counted from the model's own masks pasted again
    mask_model.half()
    n_pred_instances = pred_pixels = 0
    for (first, count), _ in loader.u8_batches():
        _, outs = mask_model.forward_tiles(loader.slide, loader.origins, first, count, loader.tile, compute_masks=True, device_outputs=False)
        for o in outs:
            o = o['det']
            if 'masks' in o:
                pm = ops.paste_label_map(o['masks'], o['boxes'], (SIDE, SIDE)).cpu().numpy()
                n_pred_instances += len(np.unique(pm[pm >= 0]))
                pred_pixels += int((pm >= 0).sum())
    mask_model.float()
    assert n_pred_instances > 0                                                     # otherwise the prediction side is vacuous
    assert masks['tp'] + masks['fn'] == int(bank.has_mask.sum()) and masks['true_sum'] == int((bank.instances != 0xFFFF).sum())
    assert masks['tp'] + masks['fp'] == n_pred_instances and masks['pred_sum'] == pred_pixels
    # the box metrics are those of the plain loader, and of a run that scores no mask
    boxes_only = lambda s: {k: v for k, v in s['det'].items() if k != 'masks'}   # noqa: E731
    assert fit_bank == fit_list and boxes_only(stats_bank) == boxes_only(stats_list) and masks == stats_list['det']['masks']
    assert fit_bank == stats_bank['det']['fitness']                                                 # the fitness stays the box fitness
    import val_nuclei
    fit_plain, stats_plain, _ = val_nuclei.run(mask_model, BankTiles(bank, BATCH, device=DEV, masks=False), half=True, device_metrics=True)
    assert 'masks' not in stats_plain['det'] and stats_plain['det'] == boxes_only(stats_bank) and fit_plain == fit_bank


# ------------------------------------------------------------------------------------------------ 6. the command line
def test_train_py_validates_on_a_held_out_bank(tmp_path, bank):
    train_path, val_path = str(tmp_path / 'train.npz'), str(tmp_path / 'held_out.npz')
    synth.synth_tile_bank(4, SIDE, NC, seed=1, instances=True).save(train_path)
    bank.save(val_path)
    cmd = [sys.executable, 'train.py', '--variant', 'n', '--nc', str(NC), '--batch-size', '4', '--imgsz', str(SIDE), '--epochs', '1', '--steps-per-epoch', '2',
           '--tile-bank', train_path, '--val-bank', val_path, '--masks', '--project', str(tmp_path), '--name', 'run', '--exist-ok', '--log-every', '1']
    p = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, YOLOv5_VERBOSE='true'), capture_output=True, text=True, timeout=240)
    out = p.stdout + p.stderr
    assert p.returncode == 0, out[-6000:]
    assert 'epochs completed' in out
    tables = re.findall(r'^\s*(\S+)\s+Labels\s+P\s+R\s+F1\s+mAP@\.5\s+mAP@\.5:\.95\s*\n\s*all\s+(\d+)\s', out, flags=re.M)
    assert [t[0] for t in tables] == ['det', 'det/mask'], out[-6000:]
    assert all(int(t[1]) == len(bank.labels) for t in tables)
    m = re.search(r'^\s*det/mask\s+Instances\s+PQ\s+SQ\s+DQ\s+AJI\s+Dice\s*\n\s*all\s+(\d+)\s', out, flags=re.M)
    assert m and int(m.group(1)) == int(bank.has_mask.sum()), out[-6000:]
