#!/usr/bin/env python3
"""Device augmentation measurements (csrc/augment.hip, metayolo.datasets.DeviceTiles) at the flagship shape: B = 64, 640 x 640, k = 2, bf16.

    python scripts/bench_augment.py [--batch 64] [--size 640] [--k 2] [--reps 30] [--steps 40] [--blocks 3] [--no-step] [--masks] [--out FILE]

(a) each kernel alone, HSV on every cell and on none: median microseconds over --reps launches (HIP events) and GB/s against the
    algorithmic bytes — the batch written once (B x 3 x S x S x 2 bytes) plus one source pixel read per output pixel (3 bytes) for the image
    kernel; the bank's boxes of the batch's cells read and the kept rows written for the box kernel;
(b) the yolov5s training step of bench.py (same model, optimizer, warm-up schedule; bench.py's own functions are imported) fed by DeviceTiles
    against the same step on bench.py's resident synthetic batch, alternated in --blocks blocks of --steps steps each in one process
    (A B A B ...), medians of the blocks;
(c) the host's cost per batch of draw_params + cell_tables (it runs beside the GPU).
With --masks the bank carries an instance map: (a) gains the three mask launches (csrc/augment_masks.hip: extents, boxes_masks, targets), and
(b) is the det + mask step (the stock graph with the mask branch) fed by DeviceTiles with masks against the same step on a resident batch of
SyntheticTiles(masks=True).
One JSON line on stdout; --out appends a readable report."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault('YOLOv5_VERBOSE', 'false')

from hd_yolo_amd import augment, ops, synth  # noqa: E402


def median_us(fn, reps, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(ts), min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--size', type=int, default=640)
    ap.add_argument('--k', type=int, default=2)
    ap.add_argument('--tiles', type=int, default=32, help='tiles of the synthetic bank')
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--steps', type=int, default=40)
    ap.add_argument('--blocks', type=int, default=3)
    ap.add_argument('--variant', default='s')
    ap.add_argument('--nc', type=int, default=8)
    ap.add_argument('--no-step', action='store_true')
    ap.add_argument('--masks', action='store_true', help='instance masks: the three mask launches and the det + mask step')
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    B, S, k = args.batch, args.size, args.k
    hyp = dict(degrees=10.0, translate=0.1, scale=0.5, shear=2.0, perspective=0.0, hsv_h=0.015, hsv_s=0.7, hsv_v=0.4, fliplr=0.5, flipud=0.5,
               transpose=0.5, cval=114, k_mosaic=k, patch_size=S, img_size=S)
    bank = synth.synth_tile_bank(args.tiles, S, args.nc, seed=0, nmin=50, nmax=200, instances=args.masks).to(dev)
    res = {'config': {'batch': B, 'size': S, 'k': k, 'bank_tiles': args.tiles, 'dtype': 'bf16', 'masks': args.masks}}

    # (c) host cost
    t0 = time.perf_counter()
    for s in range(20):
        pars = augment.draw_params(augment.step_rng(0, 0, 0, s), hyp, B, bank.n)
        tab = augment.cell_tables(pars, (S, S))
    res['host_ms_per_batch'] = round((time.perf_counter() - t0) / 20 * 1e3, 3)

    # (a) kernels alone
    out = torch.empty((B, 3, S, S), dtype=torch.bfloat16, device=dev)
    cap = B * k * k * bank.max_per_tile
    ob, ol = torch.empty((cap, 4), device=dev), torch.empty((cap,), dtype=torch.int64, device=dev)
    oi, cnt = torch.empty((cap,), device=dev), torch.empty((B + 1,), dtype=torch.int32, device=dev)
    for label, on in (('hsv_on', True), ('hsv_off', False)):
        pars['hsv'][:] = on
        tab = augment.cell_tables(pars, (S, S))
        cells, crop = torch.from_numpy(tab.cells.copy()).to(dev), torch.from_numpy(tab.crop.copy()).to(dev)
        med, best = median_us(lambda: ops.augment_tiles(bank.d_tiles, cells, crop, out, S, k, 114), args.reps)
        nbytes = B * 3 * S * S * 2 + B * S * S * 3
        res[f'tiles_{label}'] = {'median_us': round(med, 1), 'min_us': round(best, 1), 'algorithmic_mb': round(nbytes / 1e6, 1),
                                 'gb_per_s': round(nbytes / med / 1e3, 1)}
    run_boxes = lambda: ops.augment_boxes(bank.d_boxes, bank.d_labels, bank.d_offsets, len(bank.boxes), cells, crop, S, k, S, ob, ol, oi, cnt[:B], cnt[B:])
    med, best = median_us(run_boxes, args.reps)
    kept = int(cnt[:B].sum())
    cand = int(np.diff(bank.offsets)[pars['src'].reshape(-1)].sum())
    nbytes = cand * 24 + kept * 28 + B * k * k * 864
    res['boxes'] = {'median_us': round(med, 1), 'min_us': round(best, 1), 'candidates': cand, 'kept': kept, 'algorithmic_mb': round(nbytes / 1e6, 2),
                    'gb_per_s': round(nbytes / med / 1e3, 2)}

    if args.masks:
        pitch = bank.max_per_tile
        ws = torch.empty(ops.augment_mask_workspace_bytes(B * k * k, pitch), dtype=torch.uint8, device=dev)
        orf, tot = torch.empty((cap, 2), dtype=torch.int32, device=dev), torch.empty((1,), dtype=torch.int32, device=dev)
        om = torch.empty((cap, 28, 28), device=dev)
        nb = len(bank.boxes)
        launches = {
            'mask_extents': lambda: ops.augment_mask_extents(bank.d_instances, bank.d_boxes, bank.d_has_mask, bank.d_offsets, nb, cells, crop, S, k, S,
                                                             ws, pitch),
            'boxes_masks': lambda: ops.augment_boxes_masks(bank.d_boxes, bank.d_labels, bank.d_has_mask, bank.d_offsets, nb, cells, crop, S, k, S, ws,
                                                           pitch, ob, ol, oi, orf, cnt[:B], cnt[B:], tot),
            'mask_targets': lambda: ops.augment_mask_targets(bank.d_instances, bank.d_has_mask, bank.d_offsets, nb, cells, crop, S, k, S, ws, pitch, ob,
                                                             orf, tot, om)}
        for label, fn in launches.items():                      # in stream order: each launch reads what the one before wrote
            med, best = median_us(fn, args.reps)
            res[label] = {'median_us': round(med, 1), 'min_us': round(best, 1)}
        res['mask_rows'] = {'candidates': cand, 'masked_candidates': int(bank.has_mask[np.concatenate(
            [np.arange(bank.offsets[t], bank.offsets[t + 1]) for t in pars['src'].reshape(-1)])].sum()), 'kept': int(tot[0]),
            'nonzero_targets': int(om[:int(tot[0])].flatten(1).any(1).sum())}

    # (b) the training step
    if not args.no_step:
        import bench
        from metayolo.datasets import DeviceTiles
        from metayolo.models.yolo import Model
        mhyp = synth.make_hyp()
        mhyp['warmup_bias_lr'] = 0.0
        cfg = synth.make_cfg(args.variant, args.nc)
        if args.masks:
            cfg['headers'][0][3][3] = 1                          # the mask branch (one shared mask class), as train.py --masks
        model = Model(cfg, mhyp)
        model.load_state_dict(synth.mask_state_dict(model) if args.masks else synth.synth_state_dict(synth.shapes_of(model), seed=0), strict=False)
        model = model.to(dev).train()
        model.half()
        opt = bench.make_optimizer(model, mhyp, B)
        x = synth.synth_images(B, S, seed=0).to(dev)
        targets = synth.synth_targets(B, S, args.nc, seed=1, masks=args.masks)       # what SyntheticTiles(masks=...) yields for this seed
        for t in targets:
            for a in t['anns']['det']:
                a['boxes'], a['labels'] = a['boxes'].to(dev), a['labels'].to(dev)
                if args.masks:
                    a['masks'] = a['masks'].to(dev)
        nw, it = 100, [0]
        lf = lambda e: (1 - e / 300) * (1.0 - mhyp['lrf']) + mhyp['lrf']

        def step(xb, tb):
            ni = it[0]
            if ni <= nw:
                for j, g in enumerate(opt.param_groups):
                    g['lr'] = (mhyp['lr0'] * lf(0)) * ni / nw
                    g['momentum'] = mhyp['warmup_momentum'] + (mhyp['momentum'] - mhyp['warmup_momentum']) * ni / nw
            it[0] += 1
            losses, _ = model(xb, tb, compute_masks=args.masks)
            (losses['det']['det_loss'] + (losses['det']['mask_loss'] if args.masks else 0.0)).backward()
            opt.step()
            opt.zero_grad(set_to_none=True)
            return losses

        def block_resident(n):
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(n):
                step(x, targets)
            torch.cuda.synchronize()
            return (time.perf_counter() - t) / n * 1e3

        epoch = [0]

        def block_loader(n):
            loader = DeviceTiles(bank, hyp, B, n, seed=0, device=dev)
            loader.set_epoch(epoch[0])
            epoch[0] += 1
            torch.cuda.synchronize()
            t = time.perf_counter()
            for imgs, tg in loader:
                loss = step(torch.stack(list(imgs)), tg)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t) / n * 1e3
            assert torch.isfinite(loss['det']['det_loss']).all()
            return ms

        block_resident(15)
        block_loader(15)
        a, b = [], []
        for _ in range(args.blocks):
            a.append(block_resident(args.steps))
            b.append(block_loader(args.steps))
        res['step_resident_ms'] = {'blocks': [round(v, 3) for v in a], 'median': round(statistics.median(a), 3)}
        res['step_device_tiles_ms'] = {'blocks': [round(v, 3) for v in b], 'median': round(statistics.median(b), 3)}
        res['step_delta_ms'] = round(statistics.median(b) - statistics.median(a), 3)
        res['tiles_per_s_resident'] = round(B / statistics.median(a) * 1e3, 1)
        res['tiles_per_s_device_tiles'] = round(B / statistics.median(b) * 1e3, 1)
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, 'a') as f:
            f.write(f'# scripts/bench_augment.py --batch {B} --size {S} --k {k} --reps {args.reps} --steps {args.steps} --blocks {args.blocks}\n')
            for key, v in res.items():
                f.write(f'{key}: {json.dumps(v)}\n')
            f.write('\n')


if __name__ == '__main__':
    main()
