#!/usr/bin/env python3
"""Golden vectors for mask AP, from the REFERENCE's own get_mask_ious (utils_nucls.py:480-489) and APMeter (metrics.py:251-408) on the CPU:

    python tests/golden/make_golden_mask_ap.py          -> tests/golden/mask_ap.npz

Runs where make_golden.py runs (it reads the reference tree; its shims are make_golden.install_shims).  utils_nucls imports four modules
that are absent here and that get_mask_ious never touches: torchvision (already a shim), torchvision.transforms, albumentations and
DIPModels.utils_g.utils_image; they are stubbed as empty modules (transforms with a placeholder ToTensor, the one name imported from it).
The reference's metrics module calls get_mask_ious without defining it, so the script sets metrics.get_mask_ious = utils_nucls.get_mask_ious.

Inputs (tests/mask_score_ref.py makes them): 3 images of 64 x 64 label maps with 10-25 truth instances each; predictions are the truths
moved, grown or shrunk by a pixel or two, some dropped and some added, a share of disagreeing labels and the ignored label -1.  The dense
0 / 1 masks the reference is fed are (map == row).  Recorded: the label maps, labels and scores, get_mask_ious of every image, and the stats of
APMeter.add(iou_type='masks') + ap_per_class.  The inputs and IoUs are a few KB; the file is about 60 KB because the stats hold the reference's
four (3, 1000) float64 curves (py, p, r, f1), which the host test compares bit for bit.
The reference leaves ties to torch.sort, so a seed is used only if, in every image (and, for ap_per_class' own sort, over the whole
set), the scores are distinct, no prediction and no truth has two pairs of equal IoU >= 0.5, and every instance is non-empty; otherwise the next
seed is tried.  The seeds tried are recorded.  No case is dropped from a seed that passes.
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg  # noqa: E402
import mask_score_ref as ref  # noqa: E402

SHAPE, IMAGES, FIRST_SEED = (64, 64), 3, 20241018


def import_reference():
    mg.install_shims()
    for name in ('torchvision.transforms', 'albumentations', 'DIPModels', 'DIPModels.utils_g', 'DIPModels.utils_g.utils_image'):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules['torchvision.transforms'].ToTensor = object
    sys.path.insert(0, mg.REF)
    utils_nucls = importlib.import_module('utils_nucls')
    metrics = importlib.import_module('metayolo.models.metrics')
    metrics.get_mask_ious = utils_nucls.get_mask_ious
    return utils_nucls, metrics


def make_images(seed):
    rng = np.random.default_rng(seed)
    images = []
    for _ in range(IMAGES):
        n_true = int(rng.integers(10, 26))
        pm, tm, n_pred, source = ref.ellipse_pair(rng, SHAPE, n_true)
        ps, pl, tl = ref.labels_and_scores(rng, n_pred, n_true, source)
        images.append(dict(pred_map=pm, true_map=tm, scores=ps, pred_labels=pl, true_labels=tl))
    return images


def usable(images, ious):
    every = np.concatenate([im['scores'] for im in images])
    if len(np.unique(every)) != len(every):                # ap_per_class sorts the whole dataset's scores once more: no ties across images either
        return False
    for im, iou in zip(images, ious):
        n_pred, n_true = len(im['scores']), len(im['true_labels'])
        if len(np.unique(im['scores'])) != n_pred:
            return False
        if (ref.dense_masks(im['pred_map'], n_pred).sum((1, 2)) == 0).any() or (ref.dense_masks(im['true_map'], n_true).sum((1, 2)) == 0).any():
            return False
        for rows in (iou, iou.T):                          # per prediction, then per truth
            for row in rows:
                v = row[row >= np.float32(0.5)]
                if len(np.unique(v)) != len(v):
                    return False
    return True


def main():
    utils_nucls, metrics = import_reference()
    tried = []
    seed = FIRST_SEED
    while True:
        tried.append(seed)
        images = make_images(seed)
        dense = [(torch.from_numpy(ref.dense_masks(im['pred_map'], len(im['scores']))), torch.from_numpy(ref.dense_masks(im['true_map'], len(im['true_labels']))))
                 for im in images]
        ious = [utils_nucls.get_mask_ious(p, t).numpy() for p, t in dense]
        if usable(images, ious):
            break
        seed += 1
    out = {'seeds_tried': np.asarray(tried, np.int64), 'n_images': np.asarray(IMAGES)}
    meter = metrics.APMeter({1: 'a', 2: 'b', 3: 'c'})
    for i, (im, (pm, tm), iou) in enumerate(zip(images, dense, ious)):
        out[f'pred_map_{i}'], out[f'true_map_{i}'] = im['pred_map'].astype(np.int8), im['true_map'].astype(np.int8)      # fewer than 127 rows
        out[f'scores_{i}'], out[f'pred_labels_{i}'], out[f'true_labels_{i}'] = im['scores'], im['pred_labels'], im['true_labels']
        out[f'ious_{i}'] = iou.astype(np.float32)
        meter.add({'scores': torch.from_numpy(im['scores']), 'labels': torch.from_numpy(im['pred_labels']), 'masks': pm},
                  {'labels': torch.from_numpy(im['true_labels']), 'masks': tm}, iou_type='masks')
    st = meter.ap_per_class(iouv=torch.linspace(0.5, 0.95, 10))          # as the reference's caller passes it (val_nuclei.py:56)
    out['labels'], out['counts'] = np.array(st['labels']), np.array(st['counts'])
    for k in ('py', 'ap', 'p', 'r', 'f1'):
        out[k] = np.asarray(st[k], dtype=np.float64)
    path = os.path.join(HERE, 'mask_ap.npz')
    np.savez_compressed(path, **out)
    n_pairs = sum(int((iou >= 0.5).sum()) for iou in ious)
    print(f'wrote mask_ap.npz ({os.path.getsize(path)} bytes): seeds tried {tried}, pairs >= 0.5: {n_pairs}, '
          f'predictions {[len(im["scores"]) for im in images]}, truths {[len(im["true_labels"]) for im in images]}, AP@.5 {out["ap"][:, 0].round(4).tolist()}')


if __name__ == '__main__':
    main()
