"""Mask paste on the MI355X (csrc/paste.hip), measured: one label map of a slide from 10^4 .. 2.5 x 10^5 nucleus masks, and its areas.

    python scripts/bench_paste.py [--out profiles/paste_ab.txt] [--repeats 7] [--sizes 10000 100000 250000] [--loop 2000]

(a) ops.paste_label_map and ops.label_areas on synthetic slides: the detections of synth.synth_slide_truth at nucleus density (one object per
    40 x 40 px: 10^4 detections on a 3 800^2 canvas, 2.5 x 10^5 on 19 000^2) in descending score order, each with an elliptic 28 x 28
    probability patch.  Device time of each call between events (the map's fill is part of paste_label_map), and the wall time of
    evaluation.slide_label_map (both calls) between device synchronisations.  Derived: interpolated pixels per second of paste_label_map
    (about two thirds of them pass the threshold and issue an atomic) and map bytes per second of label_areas.
(b) the same map from the per-detection loop torchvision's paste_masks_in_image runs (expand, one F.interpolate per detection, threshold, a
    masked write), on the device, at --loop detections: its time, and the number of pixels on which its owners differ from the kernel's
    (torch's device interpolation is not pinned to the CPU arithmetic the kernel restates: DESIGN.md §5)."""
import argparse
import math
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import evaluation  # noqa: E402
from hd_yolo_amd import ops, synth  # noqa: E402


def stats(v):
    return f'{statistics.median(v):9.3f} [{min(v):9.3f} .. {max(v):9.3f}]'


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), r


def synth_masks(n, dev, seed, M=28):
    """(n, M, M) fp32 on the device: sigmoid of a soft ellipse that fills most of the box, as a mask head draws a nucleus"""
    g = torch.Generator(dev).manual_seed(seed)
    u = lambda lo, hi: torch.rand((n, 1, 1), device=dev, generator=g) * (hi - lo) + lo   # noqa: E731
    yy, xx = torch.meshgrid(torch.arange(M, device=dev, dtype=torch.float32), torch.arange(M, device=dev, dtype=torch.float32), indexing='ij')
    cx, cy, ax, ay, th, k = u(M * 0.42, M * 0.58), u(M * 0.42, M * 0.58), u(M * 0.3, M * 0.5), u(M * 0.3, M * 0.5), u(0, math.pi), u(3, 10)
    a = (xx - cx) * th.cos() + (yy - cy) * th.sin()
    b = -(xx - cx) * th.sin() + (yy - cy) * th.cos()
    return torch.sigmoid(k * (1 - ((a / ax) ** 2 + (b / ay) ** 2).sqrt())).contiguous()


def slide_case(n, dev):
    n_obj = max(int(n / 1.112), 1)
    side = int(math.ceil(40.0 * n_obj ** 0.5))
    _, _, pb, ps, _ = synth.synth_slide_truth(n_obj, float(side), 4, seed=1)
    order = (-ps).argsort(kind='stable')
    boxes = torch.from_numpy(pb[order]).to(dev).clamp_(0, side)
    return boxes, synth_masks(len(boxes), dev, seed=n), side


def loop_label_map(masks, boxes, size, threshold=0.5):
    """torchvision's paste_masks_in_image, one detection at a time on the device, written into one label map (rows walked from the last to the
    first, so the lowest row owns an overlap)"""
    H, W = size
    M = masks.shape[-1]
    scale = float(M + 2) / M
    padded = F.pad(masks, (1, 1, 1, 1))
    hw, hh = (boxes[:, 2] - boxes[:, 0]) * 0.5 * scale, (boxes[:, 3] - boxes[:, 1]) * 0.5 * scale
    xc, yc = (boxes[:, 2] + boxes[:, 0]) * 0.5, (boxes[:, 3] + boxes[:, 1]) * 0.5
    ib = torch.stack([xc - hw, yc - hh, xc + hw, yc + hh], 1).to(torch.int64).tolist()         # the loop's one read
    out = torch.full((H, W), -1, dtype=torch.int32, device=masks.device)
    for r in range(len(ib) - 1, -1, -1):
        x1, y1, x2, y2 = ib[r]
        w, h = max(x2 - x1 + 1, 1), max(y2 - y1 + 1, 1)
        m = F.interpolate(padded[r][None, None], size=(h, w), mode='bilinear', align_corners=False)[0, 0]
        xa, ya, xb, yb = max(x1, 0), max(y1, 0), min(x1 + w, W), min(y1 + h, H)
        if xa >= xb or ya >= yb:
            continue
        sub = out[ya:yb, xa:xb]
        sub[m[ya - y1:yb - y1, xa - x1:xb - x1] >= threshold] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='')
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--sizes', type=int, nargs='*', default=[10000, 100000, 250000])
    ap.add_argument('--loop', type=int, default=2000, help='detections of the per-detection F.interpolate loop (more is impractical)')
    opt = ap.parse_args()
    dev = torch.device('cuda', 0)
    lines = ['command: python ' + ' '.join(sys.argv), f'device: {torch.cuda.get_device_name(0)}; ms, median [min .. max] over {opt.repeats} repeats', '']
    lines.append('(a) label map and areas of a synthetic slide (28 x 28 patches, padding 1, threshold 0.5)')
    lines.append(f'{"detections":>10s} {"canvas":>8s} {"interpolated px":>16s} {"owned px":>12s}  {"paste_label_map":>34s}  {"label_areas":>34s}  '
                 f'{"slide_label_map, wall":>34s}  {"Gpx/s interp.":>13s}  {"map GB/s (areas)":>16s}')
    for n in opt.sizes:
        boxes, masks, side = slide_case(n, dev)
        R = len(boxes)
        result = {'boxes': boxes, 'masks': masks[:, None]}
        lm, areas = evaluation.slide_label_map(result, (side, side))            # warm-up
        ib = (boxes + torch.tensor([-1.0, -1.0, 1.0, 1.0], device=dev) * ((boxes[:, 2:] - boxes[:, :2]).repeat(1, 2) / 28)).to(torch.int64)
        interp = int(((ib[:, 2] - ib[:, 0] + 1).clamp(min=1) * (ib[:, 3] - ib[:, 1] + 1).clamp(min=1)).sum())       # (unclipped: a close count)
        owned = int(areas.sum())
        assert owned == int((lm >= 0).sum())
        t_map, t_area, t_all = [], [], []
        for _ in range(opt.repeats):
            t_map.append(events(lambda: ops.paste_label_map(masks, boxes, (side, side)))[0])
            t_area.append(events(lambda: ops.label_areas(lm, R))[0])
            t_all.append(wall(lambda: evaluation.slide_label_map(result, (side, side)))[0])
        lines.append(f'{R:10d} {side:8d} {interp:16d} {owned:12d}  {stats(t_map):>34s}  {stats(t_area):>34s}  {stats(t_all):>34s}  '
                     f'{interp / statistics.median(t_map) / 1e6:13.2f}  {side * side * 4 / statistics.median(t_area) / 1e6:16.1f}')
        del lm, areas, result, masks, boxes
        torch.cuda.empty_cache()
    lines.append('')
    boxes, masks, side = slide_case(opt.loop, dev)
    R = len(boxes)
    lines.append(f'(b) {R} detections on a {side} x {side} canvas: the kernel against the per-detection F.interpolate loop on the device')
    want = loop_label_map(masks, boxes, (side, side))                           # warm-up
    got = ops.paste_label_map(masks, boxes, (side, side))
    t_loop, t_kernel = [], []
    for _ in range(max(3, opt.repeats // 2)):
        t_loop.append(wall(lambda: loop_label_map(masks, boxes, (side, side)))[0])
        t_kernel.append(wall(lambda: ops.paste_label_map(masks, boxes, (side, side)))[0])
    lines.append(f'loop, wall: {stats(t_loop)}   paste_label_map, wall: {stats(t_kernel)}   ratio of medians {statistics.median(t_loop) / statistics.median(t_kernel):.0f} x')
    lines.append(f'pixels whose owner differs between the two: {int((got != want).sum())} of {int((want >= 0).sum())} owned')
    text = '\n'.join(lines)
    print(text)
    if opt.out:
        with open(opt.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
