"""Label measurement on the MI355X (csrc/measure.hip), measured: hdy_label_measure on the label map of a synthetic slide of 10^4 .. 2.5 x 10^5
nuclei, with and without the 8-bit slide under it, against hdy_label_areas on the same map (the bandwidth yardstick: the same map bytes, one
quantity per run instead of fourteen and no neighbours) and against the 14 sums written as tensor expressions (index_add_ over the owned
entries on the device: the project's usual second implementation, kept here).

    python scripts/bench_measure.py [--out profiles/measure_ab.txt] [--repeats 7] [--sizes 10000 100000 250000]

Slides at nucleus density (bench_paste.py's: one object per 40 x 40 px): the detections of synth.synth_slide_truth in descending score order,
pasted into one int32 label map with elliptic 28 x 28 patches; a random RGB slide of the same size; moments about each box's truncated corner.
The three results are checked equal before anything is timed.  Device time between events, the candidates alternating inside every repeat;
GB/s = bytes the pass has to read (map: 4 per entry, image: 3 per entry) over the median time."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

from bench_paste import events, slide_case, stats  # noqa: E402
from hd_yolo_amd import ops  # noqa: E402


def tensor_measure(lm, R, image=None, origin=None):
    """hdy_label_measure's (sums, extent) as tensor expressions on the device (include/hdyolo_measure.h, column by column)"""
    h, w = lm.shape
    dev = lm.device
    own = (lm >= 0) & (lm < R)
    ii, jj = own.nonzero(as_tuple=True)
    r = lm[ii, jj].long()
    org = torch.zeros((R, 2), dtype=torch.int64, device=dev) if origin is None else origin.long()
    dx, dy = jj - org[r, 0], ii - org[r, 1]
    pad = F.pad(lm.long(), (1, 1, 1, 1), value=1 << 40)                  # no int32 value: outside differs from everything
    c = pad[1:-1, 1:-1]
    edges = (pad[:-2, 1:-1] != c).long() + (pad[2:, 1:-1] != c) + (pad[1:-1, :-2] != c) + (pad[1:-1, 2:] != c)
    border = (ii == 0).long() + (ii == h - 1) + (jj == 0) + (jj == w - 1)
    cols = [torch.ones_like(dx), dx, dy, dx * dx, dy * dy, dx * dy, edges[ii, jj], border]
    if image is not None:
        px = image[ii, jj, :3].long()
        cols += [px[:, 0], px[:, 1], px[:, 2], px[:, 0] ** 2, px[:, 1] ** 2, px[:, 2] ** 2]
    else:
        cols += [torch.zeros_like(dx)] * 6
    sums = torch.zeros((R, 14), dtype=torch.int64, device=dev).index_add_(0, r, torch.stack(cols, 1))
    extent = torch.tensor([w, h, -1, -1], dtype=torch.int32, device=dev).repeat(R, 1)
    ji, ij = jj.int(), ii.int()
    extent[:, 0].scatter_reduce_(0, r, ji, 'amin')
    extent[:, 1].scatter_reduce_(0, r, ij, 'amin')
    extent[:, 2].scatter_reduce_(0, r, ji, 'amax')
    extent[:, 3].scatter_reduce_(0, r, ij, 'amax')
    return sums, extent


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='')
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--sizes', type=int, nargs='*', default=[10000, 100000, 250000])
    opt = ap.parse_args()
    dev = torch.device('cuda', 0)
    lines = ['command: python ' + ' '.join(sys.argv), f'device: {torch.cuda.get_device_name(0)}; device ms between events, median [min .. max] over {opt.repeats} repeats; '
             'GB/s = bytes read (map 4 B, image 3 B per entry) / median', '']
    lines.append(f'{"detections":>10s} {"canvas":>7s} {"owned":>6s}  {"label_areas (yardstick)":>34s} {"GB/s":>7s}  {"label_measure, no image":>34s} {"GB/s":>7s}  '
                 f'{"label_measure, RGB image":>34s} {"GB/s":>7s}  {"vs yardstick":>12s}  {"tensor expressions, RGB image":>34s}  {"kernel speed-up":>15s}')
    med = statistics.median
    for n in opt.sizes:
        boxes, masks, side = slide_case(n, dev)
        R = len(boxes)
        lm = ops.paste_label_map(masks, boxes, (side, side))
        del masks
        image = torch.randint(0, 256, (side, side, 3), dtype=torch.uint8, device=dev, generator=torch.Generator(dev).manual_seed(n))
        origin = boxes[:, :2].clamp(0, side - 1).to(torch.int32)
        # equal results first (and the warm-up of every candidate)
        areas = ops.label_areas(lm, R)
        s_img, e_img = ops.label_measure(lm, R, image=image, origin=origin)
        s_geo, e_geo = ops.label_measure(lm, R, origin=origin)
        s_ten, e_ten = tensor_measure(lm, R, image, origin)
        assert torch.equal(s_img, s_ten) and torch.equal(e_img, e_ten), 'the kernel and the tensor expressions differ'
        assert torch.equal(s_geo[:, :8], s_img[:, :8]) and not bool(s_geo[:, 8:].any()) and torch.equal(e_geo, e_img)
        assert torch.equal(s_img[:, 0], areas.long())
        owned = int(areas.sum()) / float(side * side)
        del s_ten, e_ten
        torch.cuda.empty_cache()
        t_area, t_geo, t_img, t_ten = [], [], [], []
        for _ in range(opt.repeats):
            t_area.append(events(lambda: ops.label_areas(lm, R))[0])
            t_geo.append(events(lambda: ops.label_measure(lm, R, origin=origin))[0])
            t_img.append(events(lambda: ops.label_measure(lm, R, image=image, origin=origin))[0])
            t_ten.append(events(lambda: tensor_measure(lm, R, image, origin))[0])
        px = side * side
        lines.append(f'{R:10d} {side:7d} {owned:6.3f}  {stats(t_area):>34s} {px * 4 / med(t_area) / 1e6:7.1f}  {stats(t_geo):>34s} {px * 4 / med(t_geo) / 1e6:7.1f}  '
                     f'{stats(t_img):>34s} {px * 7 / med(t_img) / 1e6:7.1f}  {med(t_img) / med(t_area):11.2f}x  {stats(t_ten):>34s}  {med(t_ten) / med(t_img):14.1f}x')
        del lm, image
        torch.cuda.empty_cache()
    text = '\n'.join(lines)
    print(text)
    if opt.out:
        with open(opt.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
