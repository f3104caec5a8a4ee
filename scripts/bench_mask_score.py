"""Mask scoring on the MI355X (csrc/mask_score.hip), measured: the overlap of two slide label maps of 10^4 .. 2.5 x 10^5 nuclei and the matching
on it, and a tile batch through DeviceAPMeter.add_batch_masks against the host APMeter's masks path.

    python scripts/bench_mask_score.py [--out profiles/mask_score_ab.txt] [--repeats 7] [--sizes 10000 100000 250000] [--tiles 16] [--tile 256]

(a) synthetic slides at nucleus density (bench_paste.py's: one object per 40 x 40 px): the annotations and detections of
    synth.synth_slide_truth, each side pasted into its own int32 label map with elliptic 28 x 28 patches.  Device time between events of
      - hdy_label_areas on the prediction map plus hdy_label_areas on the truth map: the YARDSTICK for the overlap launch, the same bytes
        and the same run aggregation without the pair inserts;
      - hdy_label_overlap alone (its table initialisation included), on a caller-made table;
      - ops.mask_ap_match alone;
    and the wall time of ops.label_overlap (launch, the status read, the compaction and sort) and of evaluation.score_slide_masks.
(b) --tiles tiles of --tile x --tile with about one nucleus per 40 x 40 px through DeviceAPMeter.add_batch_masks (paste, overlap, match) and
    through the host APMeter (dense 0 / 1 masks, get_mask_ious), wall time each, and whether their stats agree."""
import argparse
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

import evaluation  # noqa: E402
from bench_paste import events, stats, synth_masks, wall  # noqa: E402
from hd_yolo_amd import _lib, ops, synth  # noqa: E402
from metayolo.models.metrics import APMeter, DeviceAPMeter  # noqa: E402


def slide_case(n, dev, seed=1):
    """annotations and detections of a synthetic slide as label maps: (pred_map, true_map, scores, pred labels, truth labels, side)"""
    n_obj = max(int(n / 1.112), 1)
    side = int(math.ceil(40.0 * n_obj ** 0.5))
    tb, tl, pb, ps, pl = synth.synth_slide_truth(n_obj, float(side), 4, seed=seed)
    order = (-ps).argsort(kind='stable')
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    pred_map = ops.paste_label_map(synth_masks(len(ps), dev, seed=n), to(pb[order]).clamp_(0, side), (side, side))
    true_map = ops.paste_label_map(synth_masks(len(tl), dev, seed=n + 1), to(tb).clamp_(0, side), (side, side))
    return pred_map, true_map, to(ps[order]), to(pl[order]), to(tl), side


def raw_overlap(pm, tm, n_pred, n_true, buf, slots, parea, tarea, status):
    _lib.call('hdy_label_overlap', pm.data_ptr(), tm.data_ptr(), pm.numel(), 0, 0, None, None, n_pred, n_true, parea.data_ptr(), tarea.data_ptr(),
              buf.data_ptr(), buf.numel() * 8, slots, status.data_ptr(), ops.stream_ptr())


def tile_batch(n_tiles, tile, dev, seed):
    """per tile: the inputs of DeviceAPMeter.add_batch_masks (boxes, scores, labels, 28 x 28 masks; the truth as an instance map) and of the
    host APMeter(iou_type='masks') (dense 0 / 1 masks of the same two label maps)"""
    outs, tgts, host = [], [], []
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    dense = lambda lm, k: (lm[None] == torch.arange(k, device=dev).view(-1, 1, 1)).float().cpu()   # noqa: E731
    for i in range(n_tiles):
        tb, tl, pb, ps, pl = synth.synth_slide_truth(max(int((tile / 40.0) ** 2), 2), float(tile), 4, seed=seed + i)
        order = (-ps).argsort(kind='stable')
        boxes, masks = to(pb[order]).clamp_(0, tile), synth_masks(len(ps), dev, seed=seed + i)[:, None]
        pm = ops.paste_label_map(masks, boxes, (tile, tile))
        tm = ops.paste_label_map(synth_masks(len(tl), dev, seed=seed + 1000 + i), to(tb).clamp_(0, tile), (tile, tile))
        outs.append({'boxes': boxes, 'scores': to(ps[order]), 'labels': to(pl[order]), 'masks': masks})
        tgts.append({'labels': to(tl), 'instances': tm})
        host.append(({'scores': outs[-1]['scores'].cpu(), 'labels': outs[-1]['labels'].cpu(), 'masks': dense(pm, len(ps))},
                     {'labels': tgts[-1]['labels'].cpu(), 'masks': dense(tm, len(tl))}))
    return outs, tgts, host


def device_meter(outs, tgts, tile):
    meter = DeviceAPMeter()
    meter.add_batch_masks(outs, tgts, (tile, tile))
    return meter


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='')
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--sizes', type=int, nargs='*', default=[10000, 100000, 250000])
    ap.add_argument('--tiles', type=int, default=16)
    ap.add_argument('--tile', type=int, default=256)
    opt = ap.parse_args()
    dev = torch.device('cuda', 0)
    lines = ['command: python ' + ' '.join(sys.argv), f'device: {torch.cuda.get_device_name(0)}; ms, median [min .. max] over {opt.repeats} repeats', '']
    lines.append('(a) two label maps of a synthetic slide: overlap and matching')
    lines.append(f'{"detections":>10s} {"truths":>8s} {"canvas":>7s} {"pairs":>8s} {"mAP@.5":>7s}  {"label_areas x 2 (yardstick)":>34s}  {"hdy_label_overlap":>34s}  '
                 f'{"ratio":>6s}  {"map GB/s":>9s}  {"mask_ap_match":>34s}  {"ops.label_overlap, wall":>34s}  {"score_slide_masks, wall":>34s}')
    for n in opt.sizes:
        pm, tm, ps, pl, tl, side = slide_case(n, dev)
        R, T = len(ps), len(tl)
        st = evaluation.score_slide_masks({'label_map': pm, 'scores': ps, 'labels': pl}, {'label_map': tm, 'labels': tl})          # warm-up
        pairs, pa, ta = st['pairs'], st['pred_area'], st['true_area']
        slots = ops._pow2_at_least(4 * (R + T))
        buf, _, _ = ops._overlap_table(slots, dev)
        parea, tarea, status = torch.empty_like(pa), torch.empty_like(ta), torch.empty((2,), dtype=torch.int32, device=dev)
        raw_overlap(pm, tm, R, T, buf, slots, parea, tarea, status)
        assert status.tolist() == [len(pairs), 0] and torch.equal(parea, pa) and torch.equal(tarea, ta)
        assert torch.equal(pa, ops.label_areas(pm, R)) and torch.equal(ta, ops.label_areas(tm, T))
        t_area, t_over, t_match, t_wrap, t_all = [], [], [], [], []
        for _ in range(opt.repeats):
            t_area.append(events(lambda: (ops.label_areas(pm, R), ops.label_areas(tm, T)))[0])
            t_over.append(events(lambda: raw_overlap(pm, tm, R, T, buf, slots, parea, tarea, status))[0])
            t_match.append(events(lambda: ops.mask_ap_match(pairs, pa, ta, ps, pl, tl, np.linspace(0.5, 0.95, 10).astype(np.float32)))[0])
            t_wrap.append(wall(lambda: ops.label_overlap(pm, tm, R, T))[0])
            t_all.append(wall(lambda: evaluation.score_slide_masks({'label_map': pm, 'scores': ps, 'labels': pl}, {'label_map': tm, 'labels': tl}))[0])
        med = statistics.median
        lines.append(f'{R:10d} {T:8d} {side:7d} {len(pairs):8d} {float(st["ap"][:, 0].mean()):7.4f}  {stats(t_area):>34s}  {stats(t_over):>34s}  '
                     f'{med(t_over) / med(t_area):6.2f}  {2 * side * side * 4 / med(t_over) / 1e6:9.1f}  {stats(t_match):>34s}  {stats(t_wrap):>34s}  {stats(t_all):>34s}')
        del pm, tm, buf, st, pairs
        torch.cuda.empty_cache()
    lines.append('')
    lines.append(f'(b) {opt.tiles} tiles of {opt.tile} x {opt.tile}: DeviceAPMeter.add_batch_masks (a paste per tile, one overlap with per-tile bases, one matching call) against the host APMeter (dense masks)')
    outs, tgts, host = tile_batch(opt.tiles, opt.tile, dev, seed=100)
    device_meter(outs, tgts, opt.tile)                                           # warm-up
    t_dev, t_host = [], []
    for _ in range(max(3, opt.repeats // 2)):
        t, meter = wall(lambda: device_meter(outs, tgts, opt.tile))
        t_dev.append(t)

        def run_host():
            m = APMeter()
            for o, tg in host:
                m.add(o, tg, iou_type='masks')
            return m
        t, hm = wall(run_host)
        t_host.append(t)
    got, want = meter.ap_per_class(), hm.ap_per_class(iouv=torch.linspace(0.5, 0.95, 10))
    same = all(np.array_equal(got[k], want[k]) for k in ('ap', 'p', 'r', 'f1', 'py'))
    lines.append(f'{sum(len(o["scores"]) for o in outs)} detections x {sum(len(t["labels"]) for t in tgts)} truths: device, wall {stats(t_dev)}   host APMeter, wall {stats(t_host)}   '
                 f'ratio of medians {statistics.median(t_host) / statistics.median(t_dev):.0f} x   stats equal: {same}   mAP@.5 {float(got["ap"][:, 0].mean()):.4f}')
    text = '\n'.join(lines)
    print(text)
    if opt.out:
        with open(opt.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
