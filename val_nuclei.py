#!/usr/bin/env python3
"""Validation entry point with the reference's `run(model, dataloader, meta_info, callbacks, ...)` surface
(reference: val_nuclei.py:108-221), on the MI355X path: eval forward (HIP plan) -> decode + NMS kernels -> APMeter.

    python val_nuclei.py --variant s --nc 8 --imgsz 640 --batch-size 32 --batches 4 [--device-metrics]
    python val_nuclei.py --variant s --nc 8 --weights best.pt --tile-bank held_out.npz [--masks]
"""
import argparse
import os
import sys

import numpy as np
os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')               # before the HIP runtime loads: see hd_yolo_amd/__init__.py
os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from metayolo import LOGGER  # noqa: E402
from metayolo.engines.torch_utils import select_device, time_sync, to_device  # noqa: E402
from metayolo.models.metrics import APMeter, DeviceAPMeter  # noqa: E402


class _NoCallbacks:
    def run(self, *a, **k):
        pass


def flatten_onehot_objects(x):
    """(n, nc+1) multi-hot labels -> one row per (object, class) pair (reference val_nuclei.py:34-49)."""
    nbox, nc = x['labels'].shape
    keep = x['labels'].flatten() > 0.
    res = dict(x)
    res['labels'] = torch.tile(torch.arange(nc, device=x['labels'].device), (nbox,))[keep]
    res['labels'][res['labels'] == 0] = -100
    res['boxes'] = torch.repeat_interleave(x['boxes'], nc, 0)[keep]
    if 'scores' in x:
        res['scores'] = x['scores'].flatten()[keep]
    return res


def summarize_stats(ap_meter, task_id, **kwargs):
    """Precision / recall / F1 at the best mean-F1 operating point, AP@.5 and AP@.5:.95 per class; the summary averages the
    first four classes only, as the reference does for the NuCLS label set (val_nuclei.py:51-93)."""
    stats = ap_meter.ap_per_class(iouv=torch.linspace(0.5, 0.95, 10), ignore=[-100, -1])
    names = ap_meter.labels_text
    LOGGER.info(('%10s' * 2 + '%12s' * 5) % (task_id, 'Labels', 'P', 'R', 'F1', 'mAP@.5', 'mAP@.5:.95'))
    if not len(stats['labels']):
        return {'mp': 0.0, 'mr': 0.0, 'f1': 0.0, 'map50': 0.0, 'map': 0.0, 'fitness': 0.0}
    idx = stats['f1'].mean(0).argmax()
    p, r, f1 = stats['p'][:, idx], stats['r'][:, idx], stats['f1'][:, idx]
    ap50, ap = stats['ap'][:, 0], stats['ap'].mean(1)
    map50, map_ = float(ap50[:4].mean()), float(ap[:4].mean())
    mp, mr, mf1 = float(p[:4].mean()), float(r[:4].mean()), float(f1[:4].mean())
    pf = '%10s' + '%10i' + '%12.3g' * 5
    LOGGER.info(pf % ('all', sum(stats['counts']), mp, mr, mf1, map50, map_))
    for i, c in enumerate(stats['labels']):
        LOGGER.info(pf % (names.get(c, str(c)), stats['counts'][i], p[i], r[i], f1[i], ap50[i], ap[i]))
    return {'mp': mp, 'mr': mr, 'f1': mf1, 'map50': map50, 'map': map_, 'fitness': map50 * 0.1 + map_ * 0.9}


def _pixel_boxes(boxes, counts, w, h):
    """run()'s per-image rule `max(boxes) <= 1.0: normalised training boxes -> pixels` for a whole batch of truths (boxes concatenated,
    `counts` rows per image) as one segmented reduction on the device, no read: every image's boxes times (w, h, w, h) or times 1."""
    dev = boxes.device
    image = torch.repeat_interleave(torch.arange(len(counts), device=dev), torch.tensor(counts, device=dev), output_size=int(sum(counts)))
    top = torch.full((len(counts),), float('-inf'), dtype=boxes.dtype, device=dev)
    top = top.scatter_reduce(0, image, boxes.reshape(len(boxes), -1).max(1).values, 'amax')
    scale = torch.where((top <= 1.0)[image, None], boxes.new_tensor([w, h, w, h]), boxes.new_ones(4))
    return boxes * scale


def _add_batch_on_device(meter, outputs, targets, task_id, w, h):
    """one batch of one single-label task into a DeviceAPMeter: no device-to-host read"""
    outs = [output[task_id] for output in outputs]
    tgts = [target['anns'][task_id][0] for target in targets]
    counts = [len(t['labels']) for t in tgts]
    if sum(counts):
        boxes = _pixel_boxes(torch.cat([t['boxes'].reshape(-1, 4) for t in tgts]), counts, w, h).split(counts)
    else:
        boxes = [t['boxes'] for t in tgts]
    meter.add_batch(outs, [{'boxes': b, 'labels': t['labels']} for b, t in zip(boxes, tgts)])


def max_stride(model):
    """the largest stride of any header's levels: what a tile side must be a multiple of"""
    return int(max(h._stride_cached(i) for h in model.headers.values() for i in range(h.nl)))


def _add_batch_masks_on_device(meter, outputs, targets, task_id, size):
    """one batch of one task into its mask meter (DeviceAPMeter.add_batch_masks); an image without detections comes without 'masks'"""
    outs = []
    for output in outputs:
        o = output[task_id]
        outs.append(o if 'masks' in o else dict(o, masks=o['boxes'].new_zeros((len(o['boxes']), 1, 28, 28))))
    tgts = [{'labels': a['labels'], 'instances': a['instances']} for a in (target['anns'][task_id][0] for target in targets)]
    meter.add_batch_masks(outs, tgts, size)


def summarize_masks(mask_meter, task_id):
    """the mask table of one task: summarize_stats on mask IoU, then PQ / SQ / DQ / AJI / Dice of the pooled segmentations"""
    stats = summarize_stats(mask_meter, task_id=f'{task_id}/mask')
    seg = mask_meter.segmentation_summary()
    LOGGER.info(('%10s' * 2 + '%12s' * 5) % (f'{task_id}/mask', 'Instances', 'PQ', 'SQ', 'DQ', 'AJI', 'Dice'))
    LOGGER.info(('%10s' + '%10i' + '%12.3g' * 5) % ('all', seg['tp'] + seg['fn'], seg['pq'], seg['sq'], seg['dq'], seg['aji'], seg['dice']))
    return {**stats, **seg}


@torch.no_grad()
def run(model, dataloader, meta_info=None, callbacks=None, batch_size=32, half=True, verbose=False, save_txt=False,
        save_dir='', plots=False, epoch=0, device_metrics=False):
    """device_metrics=True: the tasks whose header is single-label are scored by DeviceAPMeter (the matching on the device, one call per
    batch, no device-to-host read in the loop); the others, and everything by default, by the host APMeter.  Return values and the log
    table are the same in both modes.

    A metayolo.datasets.BankTiles loader runs through the 8-bit path: every batch is gathered from the bank straight into the plan's input
    buffer (Model.forward_tiles), no float batch is made, and the detections are bit-identical to those of the loader's float tuples.  Its
    tile sides must be multiples of the model's largest stride (ValueError).

    Masks are scored for a task when the model's only header has a mask branch, the task is scored on the device and every target of the
    batch carries 'instances' (BankTiles on a bank with an instance map): the forward then runs with compute_masks=True and a second
    DeviceAPMeter receives add_batch_masks.  val_stats[task]['masks'] then holds summarize_stats' six keys on mask IoU plus pq, sq, dq, aji,
    dice and the counts behind them (DeviceAPMeter.segmentation_summary), with one more log table; every other key, and fitness, stay the box
    metrics.  The segmentation that PQ / AJI / Dice judge is everything the model outputs at its conf_thres, pasted in score order: at the
    AP-style threshold of 0.001 the low-score rows count as instances and own pixels too."""
    from metayolo.datasets import BankTiles
    callbacks = callbacks or _NoCallbacks()
    device = next(model.parameters()).device
    model.half() if half else model.float()
    model.eval()
    names = lambda task_id: (meta_info or {}).get(task_id, {}).get('labels_text', {})   # noqa: E731
    on_device = {task_id: bool(device_metrics) and not getattr(h, 'multi_label', False) for task_id, h in model.headers.items()}
    meters = {task_id: (DeviceAPMeter if on_device[task_id] else APMeter)(names(task_id)) for task_id in model.headers}
    # (the mask branch of a plan belongs to its only header, as in Model._forward_headers)
    mask_tasks = [task_id for task_id, h in model.headers.items() if on_device[task_id] and getattr(h, 'nc_masks', 0) > 0 and len(model.headers) == 1]
    mask_meters = {}
    from_bank = isinstance(dataloader, BankTiles)
    if from_bank:
        dataloader.check_stride(max_stride(model))
    callbacks.run('on_val_start')
    dt, n_image = [0.0, 0.0, 0.0], 0
    for batch_i, (imgs, targets) in enumerate(dataloader.u8_batches() if from_bank else dataloader):
        callbacks.run('on_val_batch_start')
        t1 = time_sync()
        if from_bank:
            (first, count), (h, w) = imgs, dataloader.tile
        else:
            imgs = torch.stack(list(imgs)).to(device, non_blocking=True).float()
            h, w = imgs.shape[-2:]
        targets = to_device(targets, device)
        with_masks = [task_id for task_id in mask_tasks if all('instances' in t['anns'][task_id][0] for t in targets)]
        t2 = time_sync()
        dt[0] += t2 - t1
        if from_bank:
            _, outputs = model.forward_tiles(dataloader.slide, dataloader.origins, first, count, (h, w), compute_masks=bool(with_masks),
                                             device_outputs=False)
        else:
            _, outputs = model(imgs, compute_masks=bool(with_masks))
        t3 = time_sync()
        dt[1] += t3 - t2
        for task_id in model.headers:
            if on_device[task_id]:
                _add_batch_on_device(meters[task_id], outputs, targets, task_id, w, h)
        for task_id in with_masks:
            if task_id not in mask_meters:
                mask_meters[task_id] = DeviceAPMeter(names(task_id))
            _add_batch_masks_on_device(mask_meters[task_id], outputs, targets, task_id, (h, w))
        for output, target in zip(outputs, targets):
            n_image += 1
            for task_id in model.headers:
                if on_device[task_id]:
                    continue
                o, t = output[task_id], dict(target['anns'][task_id][0])
                if t['boxes'].numel() and float(t['boxes'].max()) <= 1.0:      # normalised training boxes -> pixels
                    t['boxes'] = t['boxes'] * t['boxes'].new_tensor([w, h, w, h])
                if o['labels'].dim() == 2:
                    o = flatten_onehot_objects(o)
                if t['labels'].dim() == 2:
                    t = flatten_onehot_objects(t)
                meters[task_id].add(o, t, iou_type='boxes')
        dt[2] += time_sync() - t3
        callbacks.run('on_val_batch_end')
    speeds = tuple(x / max(n_image, 1) * 1e3 for x in dt)
    val_stats = {task_id: summarize_stats(m, task_id=task_id) for task_id, m in meters.items()}
    fitness = sum(s['fitness'] for s in val_stats.values())
    for task_id, m in mask_meters.items():
        val_stats[task_id]['masks'] = summarize_masks(m, task_id)
    model.float()
    return fitness, val_stats, speeds


def load_val_bank(path, nc, batch_size, device, task, masks):
    """--tile-bank / --val-bank: the bank as a BankTiles loader; a bank whose labels pass the model's nc is refused"""
    from hd_yolo_amd.augment import TileBank
    from metayolo.datasets import BankTiles
    bank = TileBank.load(path)
    if bank.nc > nc:
        raise SystemExit(f'tile bank {path} holds labels up to {bank.nc}, the model has nc={nc}')
    return BankTiles(bank, batch_size, device=device, task=task, masks=masks)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--variant', default='s')
    ap.add_argument('--nc', type=int, default=8)
    ap.add_argument('--imgsz', type=int, default=640)
    ap.add_argument('--batch-size', type=int, default=32)
    ap.add_argument('--batches', type=int, default=4)
    ap.add_argument('--weights', default='')
    ap.add_argument('--device', default='')
    ap.add_argument('--no-half', action='store_true')
    ap.add_argument('--device-metrics', action='store_true', help='score single-label tasks on the device (DeviceAPMeter) instead of the host APMeter')
    ap.add_argument('--tile-bank', default='', help='.npz tile bank (hd_yolo_amd.augment.TileBank) to validate on, at its own tile size, through the 8-bit '
                                                   'path and the device metrics, instead of synthetic tiles')
    ap.add_argument('--masks', action='store_true', help='--tile-bank: a model with the mask branch; a bank with an instance map is also scored on mask '
                                                         'IoU (mask mAP, PQ / SQ / DQ / AJI / Dice)')
    opt = ap.parse_args()
    if opt.masks and not opt.tile_bank:
        ap.error('--masks needs --tile-bank')
    from hd_yolo_amd import synth
    from metayolo.datasets import SyntheticTiles
    from metayolo.models.yolo import Model
    device = select_device(opt.device)
    cfg = synth.make_cfg(opt.variant, opt.nc)
    if opt.masks:
        cfg['headers'][0][3][3] = 1                           # stock graph + the mask branch (one shared mask class), as train.py --masks
    model = Model(cfg, synth.make_hyp())
    if opt.weights:
        from metayolo.engines.general import checkpoint_state, intersect_dicts
        ck = torch.load(opt.weights, map_location='cpu', weights_only=False)
        sd = checkpoint_state(ck, prefer_ema=True)        # this build's or the reference's checkpoint form; EMA weights as val.run gets them in train.py:487
        model.load_state_dict(intersect_dicts(sd, model.state_dict()), strict=False)
    else:
        model.load_state_dict(synth.synth_state_dict(synth.shapes_of(model), seed=0), strict=False)
    model = model.to(device)
    if opt.tile_bank:
        task = next(iter(model.headers))
        loader = load_val_bank(opt.tile_bank, opt.nc, opt.batch_size, device, task, opt.masks)
        try:
            loader.check_stride(max_stride(model))
        except ValueError as e:
            raise SystemExit(str(e))
        LOGGER.info(f'--tile-bank: --imgsz is ignored, the inference size is the tile size {loader.tile[0]} x {loader.tile[1]} of {opt.tile_bank}')
        fitness, stats, speeds = run(model, loader, half=not opt.no_half, device_metrics=True)
    else:
        loader = SyntheticTiles(opt.batch_size, opt.imgsz, opt.nc, opt.batches, seed=12345)
        fitness, stats, speeds = run(model, loader, half=not opt.no_half, device_metrics=opt.device_metrics)
    print(f'fitness {fitness:.4f}; ms/img pre {speeds[0]:.3f} infer+nms {speeds[1]:.3f} metrics {speeds[2]:.3f}')


if __name__ == '__main__':
    main()
