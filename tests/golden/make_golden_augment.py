#!/usr/bin/env python3
"""Golden vectors for the target side of the device augmentation, from the REFERENCE's own code -> tests/golden/augment.npz.

    python tests/golden/make_golden_augment.py

Runs where make_golden.py runs (it reads the reference checkout that script names); the test-suite only sees the .npz.  The reference's
metayolo/datasets.py and metayolo/engines/image_utils.py are imported unmodified under make_golden.py's shims plus the ones below, and
every target of a case is produced by the reference's functions, called in the order of TorchDataset.__getitem__'s training branch:

    random_projective (random_transform_pars, estimate_matrix, warp_coords, Mask(clip=True).box, box_candidates)
    -> hflip / vflip / transpose_image_target (the three *_annotation flips; random_flip's own coin tosses are replaced by chosen flags so
       that every combination occurs) -> pad_image_target (mosaic offset) -> merge_annotations
    -> get_crop_width(pos='random') + crop_image_target (crop_annotation, remove_invalid_objects)
    -> remove_invalid_objects with the final 10 px filter -> target_to_tensors(normalize_box=True).

Shims that are restatements, not reference code: cv2.getRotationMatrix2D (OpenCV's documented formula), skimage.util.crop (array slicing),
cv2.warpAffine / warpPerspective (return an empty canvas: the goldens cover targets only; the image arithmetic is pinned by
tests/augment_ref.py and known-answer cases, the cv2 boundary being unpinned).

Every source box carries a unique label, so keep / drop decisions and order can be read off the labels.  Inputs are redrawn until, in the
reference's float64 result, no box lies within 0.01 px of a size threshold (2 px in box_candidates, 10 px in the final filter, 0 px in the
crop's filter) or within 1e-3 of the area-ratio (0.1) and aspect (100) thresholds: the generator asserts this.
"""
import importlib
import math
import os
import random
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

OUT = os.path.join(HERE, 'augment.npz')


def install_augment_shims():
    mg.install_shims()
    cv2 = sys.modules['cv2']
    cv2.INTER_NEAREST, cv2.INTER_LINEAR, cv2.INTER_CUBIC = 0, 1, 2

    def get_rotation_matrix_2d(angle, center, scale):          # restatement of OpenCV's documented formula
        a, b = scale * math.cos(angle * math.pi / 180), scale * math.sin(angle * math.pi / 180)
        return np.array([[a, b, (1 - a) * center[0] - b * center[1]], [-b, a, b * center[0] + (1 - a) * center[1]]])

    def warp(img, M, dsize, flags=None, borderValue=None):
        return np.zeros((dsize[1], dsize[0]) + img.shape[2:], img.dtype)

    cv2.getRotationMatrix2D, cv2.warpAffine, cv2.warpPerspective = get_rotation_matrix_2d, warp, warp
    sk = types.ModuleType('skimage')
    sk.__path__, sk.__version__ = [], '0.19.0'
    for sub in ('io', 'util', 'transform', 'morphology', 'color'):
        m = types.ModuleType('skimage.' + sub)
        setattr(sk, sub, m)
        sys.modules['skimage.' + sub] = m
    for name in ('rgb2hsv', 'hsv2rgb', 'hed2rgb', 'rgb2hed', 'gray2rgb'):
        setattr(sk.color, name, None)

    def crop(ar, crop_width, copy=False, order='K'):           # restatement: skimage.util.crop is array slicing
        sl = tuple(slice(int(a), ar.shape[i] - int(b)) for i, (a, b) in enumerate(crop_width))
        return ar[sl]

    sk.util.crop = crop
    sys.modules['skimage'] = sk
    tv = sys.modules['torchvision']
    tr = types.ModuleType('torchvision.transforms')
    tr.ToTensor = object
    rh = types.ModuleType('torchvision.models.detection.roi_heads')
    rh.paste_masks_in_image = None
    tv.transforms = tr
    sys.modules['torchvision.transforms'], sys.modules['torchvision.models.detection.roi_heads'] = tr, rh
    tu = types.ModuleType('metayolo.engines.torch_utils')
    tu.collate_fn = tu.torch_distributed_zero_first = None
    sys.modules['metayolo.engines.torch_utils'] = tu
    return importlib.import_module('metayolo.datasets')


def source_boxes(rng, m, tile):
    c = rng.uniform(0.05 * tile, 0.95 * tile, (m, 2))
    wh = rng.uniform(0.15 * tile, 0.45 * tile, (m, 2))
    return np.clip(np.concatenate([c - wh / 2, c + wh / 2], 1), 0, tile).astype(np.float32)


def margins_ok(rec, final_in, S):
    for box1, box2 in rec:
        w1, h1 = box1[2] - box1[0], box1[3] - box1[1]
        w2, h2 = box2[2] - box2[0], box2[3] - box2[1]
        if (np.abs(w2 - 2) < 0.01).any() or (np.abs(h2 - 2) < 0.01).any():
            return False
        ratio = w2 * h2 / (w1 * h1 + 1e-16)
        ar = np.maximum(w2 / (h2 + 1e-16), h2 / (w2 + 1e-16))
        live = (w2 > 2) & (h2 > 2)
        if (np.abs(ratio - 0.1)[live] < 1e-3).any() or (np.abs(ar - 100)[live] < 1e-3).any():
            return False
    b = np.clip(final_in, 0, S)
    w, h = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    return not ((np.abs(w - 10) < 0.01).any() or (np.abs(h - 10) < 0.01).any())


def run_case(ds, seed, tile, patch, k, S, hyp, per_cell):
    """one output image through the reference; returns None when a threshold margin is violated"""
    random.seed(seed)
    np.random.seed(seed)
    rng = np.random.default_rng(seed)
    hyp = dict(hyp, patch_size=patch)
    pars_rec, cand_rec = [], []
    orig_pars, orig_cand = ds.random_transform_pars, ds.box_candidates

    def rec_pars(*a, **kw):
        pars_rec.append(orig_pars(*a, **kw))
        return pars_rec[-1]

    def rec_cand(box1, box2, **kw):
        cand_rec.append((np.array(box1, np.float64), np.array(box2, np.float64)))
        return orig_cand(box1=box1, box2=box2, **kw)

    ds.random_transform_pars, ds.box_candidates = rec_pars, rec_cand
    try:
        cells, ann_list, label0 = [], [], 1
        image = np.zeros((tile, tile, 3), np.uint8)
        for rc in range(k * k):
            r, c = rc // k, rc % k
            boxes = source_boxes(rng, per_cell, tile)
            labels = np.arange(label0, label0 + per_cell)
            label0 += per_cell
            flips = [bool(v) for v in rng.integers(0, 2, 3)]
            target = {'anns': {'det': [{'boxes': torch.as_tensor(boxes), 'labels': torch.as_tensor(labels), 'masks': [None] * per_cell}]}}
            img, tgt = ds.random_projective(image, target, hyp, output_shape=patch, cval=0)
            canvas_boxes = tgt['anns']['det'][0]['boxes'].numpy().copy()
            canvas_labels = tgt['anns']['det'][0]['labels'].numpy().copy()
            if flips[0]:
                img, tgt = ds.hflip_image_target(img, tgt)
            if flips[1]:
                img, tgt = ds.vflip_image_target(img, tgt)
            if flips[2]:
                img, tgt = ds.transpose_image_target(img, tgt)
            pad_var = [(r * patch, (k - 1 - r) * patch), (c * patch, (k - 1 - c) * patch)]
            _, tgt = ds.pad_image_target(None, tgt, pad_var, mode='constant')
            ann_list.extend(tgt['anns']['det'])
            M = ds.estimate_matrix(pars_rec[-1])
            cells.append({'boxes': boxes, 'labels': labels, 'flips': flips, 'pars': pars_rec[-1], 'M': M, 'canvas_boxes': canvas_boxes,
                          'canvas_labels': canvas_labels})
        ann_list = [a for a in ann_list if len(a['boxes'])]
        size = (k * patch, k * patch)
        mosaic = np.zeros(size + (3,), np.uint8)
        target = {'image_id': 0, 'size': size, 'anns': ds.merge_annotations({'det': ann_list}, size)}
        crop_width = ds.get_crop_width(mosaic.shape, output_size=ds.get_size(S), pos='random')      # as crop_image_target_if_needed calls it
        image, target = ds.crop_image_target(mosaic, target, crop_width, remove_invalid=True)
        before = np.asarray(target['anns']['det'][0]['boxes'], np.float64).copy()
        filter_fn = lambda x: (x['boxes'][:, 0] < x['boxes'][:, 2] - 10) & (x['boxes'][:, 1] < x['boxes'][:, 3] - 10)      # noqa: E731 (datasets.py, final filter)
        target['anns'] = {kk: [ds.remove_invalid_objects(ann, image.shape, filter_fn=filter_fn) for ann in v] for kk, v in target['anns'].items()}
        pix = np.asarray(target['anns']['det'][0]['boxes'], np.float64).copy()
        final = ds.target_to_tensors(target, normalize_box=True)['anns']['det'][0]
    finally:
        ds.random_transform_pars, ds.box_candidates = orig_pars, orig_cand
    if not margins_ok(cand_rec, before, S):
        return None
    crop = (int(crop_width[1][0]), int(crop_width[0][0]))
    assert image.shape[:2] == (S, S)
    return {'cells': cells, 'crop': crop, 'pix': pix, 'final': final['boxes'].numpy(), 'labels': final['labels'].numpy()}


CASES = {
    # name: (tile, patch, k, S, boxes per cell, hyp)
    'affine_k2': (64, 80, 2, 112, 12, dict(degrees=20.0, translate=0.1, scale=0.3, shear=6.0, perspective=0.0)),
    'perspective_k1': (96, 96, 1, 96, 24, dict(degrees=10.0, translate=0.35, scale=0.4, shear=4.0, perspective=0.001)),
    'affine_k3_big_crop': (48, 64, 3, 100, 8, dict(degrees=45.0, translate=0.2, scale=0.5, shear=10.0, perspective=0.0)),
    'perspective_k2': (64, 64, 2, 128, 12, dict(degrees=15.0, translate=0.15, scale=0.3, shear=5.0, perspective=0.002)),
}
PAR_KEYS = ('c_x', 'c_y', 'p_x', 'p_y', 'angle', 'scale', 'shear_x', 'shear_y', 't_x', 't_y')


def main():
    ds = install_augment_shims()
    out = {'names': np.array(sorted(CASES))}
    for name in sorted(CASES):
        tile, patch, k, S, per_cell, hyp = CASES[name]
        res, seed = None, 0
        while res is None:
            seed += 1
            assert seed < 200, name
            res = run_case(ds, 1000 + seed, tile, patch, k, S, hyp, per_cell)
        kept = len(res['pix'])
        assert 0 < kept < k * k * per_cell, (name, kept)
        out[f'{name}/shape'] = np.array([tile, patch, k, S, per_cell], np.int64)
        out[f'{name}/crop'] = np.array(res['crop'], np.int64)
        out[f'{name}/boxes'] = np.stack([c['boxes'] for c in res['cells']])
        out[f'{name}/src_labels'] = np.stack([c['labels'] for c in res['cells']])
        out[f'{name}/flips'] = np.array([c['flips'] for c in res['cells']])
        out[f'{name}/pars'] = np.array([[c['pars'][key] for key in PAR_KEYS] for c in res['cells']], np.float64)
        out[f'{name}/M'] = np.stack([c['M'] for c in res['cells']])
        for j, c in enumerate(res['cells']):
            out[f'{name}/canvas_boxes/{j}'] = c['canvas_boxes']
            out[f'{name}/canvas_labels/{j}'] = c['canvas_labels']
        out[f'{name}/pix'], out[f'{name}/final'], out[f'{name}/labels'] = res['pix'], res['final'], res['labels']
        print(f'{name}: seed {1000 + seed}, {kept} of {k * k * per_cell} boxes kept, crop {res["crop"]}')
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
