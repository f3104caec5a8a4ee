"""Neighbourhood features on the MI355X (csrc/spatial.hip), measured: hdy_spatial_neighbors alone, hdy_spatial_cells alone and the whole
ops.spatial_neighbors call (cell ids, the stable device sort, packing and both launches) on synthetic slides of 10^4 .. 2.5 x 10^5 nuclei,
against the same counts written as chunked dense tensor expressions on the device (a chunk x N int64 distance block per step: the N x N
matrix that cannot exist at slide size, walked in slices).

    python scripts/bench_spatial.py [--out profiles/spatial_ab.txt] [--repeats 7] [--sizes 10000 100000 250000] [--dense-budget 60]

Slides at nucleus density (one object per 40 x 40 px): the box centres of synth.synth_slide_truth's detections, C = 3 classes, radii 16 / 32 / 64
px.  The dense yardstick runs in the same process and alternates with the kernel inside every repeat; its first chunks are timed and the run
is made only where the extrapolated time of all its repeats stays within --dense-budget seconds ("not run" otherwise).  Where it runs, its
counts are checked equal to the kernel's before anything is timed.  Device time between events; the two kernels alone are timed as INNER
back-to-back calls per repeat and reported per call, which at the small sizes is what the host needs to issue a call, not the kernel."""
import argparse
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

from bench_paste import events, stats  # noqa: E402
from hd_yolo_amd import ops, spatial, synth  # noqa: E402

C = 3
RADII_PX = (16, 32, 64)
INNER = 20          # back-to-back calls per timed window of a kernel alone


def dense_counts(xy, cls, radii, chunk, first=None):
    """counts (N, K, C) by dense tensor expressions: per chunk of queries one (chunk, N) int64 block of squared distances"""
    N = xy.shape[0]
    x, y = xy[:, 0].long(), xy[:, 1].long()
    onehot = torch.stack([cls == c for c in range(C)], 1).to(torch.float64)          # (N, C): the class sums as one matrix product per radius
    out = torch.zeros((N, len(radii), C), dtype=torch.int32, device=xy.device)
    for n, q0 in enumerate(range(0, N, chunk)):
        if first is not None and n >= first:
            break
        q = slice(q0, min(q0 + chunk, N))
        dx, dy = x[q, None] - x[None, :], y[q, None] - y[None, :]
        d2 = dx * dx + dy * dy
        for k, r in enumerate(radii):
            out[q, k] = ((d2 <= r * r).to(torch.float64) @ onehot).to(torch.int32)     # exact: counts < 2^53
    out -= torch.nn.functional.one_hot(cls.long(), C).to(torch.int32)[:, None, :]      # a point is not its own neighbour
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='')
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--sizes', type=int, nargs='*', default=[10000, 100000, 250000])
    ap.add_argument('--dense-budget', type=float, default=60.0, help='seconds all repeats of the dense yardstick may take at one size')
    opt = ap.parse_args()
    dev = torch.device('cuda', 0)
    radii = [spatial.radius_units(r) for r in RADII_PX]
    lines = ['command: python ' + ' '.join(sys.argv),
             f'device: {torch.cuda.get_device_name(0)}; device ms between events, median [min .. max] over {opt.repeats} repeats; C = {C}, radii {RADII_PX} px',
             f'hdy_spatial_cells / hdy_spatial_neighbors: per call, {INNER} back-to-back calls per window (host issue time included)',
             'form of hdy_spatial_neighbors: one lane per query, candidates straight from global memory (the LDS-staged form was not built)', '']
    lines.append(f'{"nuclei":>8s} {"side px":>8s} {"cells":>11s} {"mean nb 64px":>12s}  {"hdy_spatial_cells":>34s}  {"hdy_spatial_neighbors":>34s}  '
                 f'{"ops.spatial_neighbors (whole call)":>34s}  {"dense tensor expressions":>34s}  {"whole call vs dense":>19s}')
    med = statistics.median
    for n in opt.sizes:
        n_obj = max(int(n / 1.112), 1)
        side = int(math.ceil(40.0 * n_obj ** 0.5))
        _, _, pb, _, pl = synth.synth_slide_truth(n_obj, float(side), C, seed=1)
        boxes = torch.from_numpy(pb).to(dev)
        xy = spatial.to_units(torch.stack([(boxes[:, 0] + boxes[:, 2]) * 0.5, (boxes[:, 1] + boxes[:, 3]) * 0.5], 1).clamp(0, side))
        cls = (torch.from_numpy(pl).to(dev) - 1).to(torch.int32)
        N = xy.shape[0]
        info = {}
        counts, d2, row = ops.spatial_neighbors(xy, cls, C, radii, info=info)
        assert int(info['status']) == 0
        pts, cell_start, cell, ncx, ncy = (info[k] for k in ('pts', 'cell_start', 'cell_units', 'ncx', 'ncy'))
        sorted_call = lambda: ops.spatial_neighbors_sorted(pts, cell_start, cell, ncx, ncy, radii, C)      # noqa: E731
        again = sorted_call()
        assert all(torch.equal(a, b) for a, b in zip(again, (counts, d2, row)))
        # the yardstick: is it affordable here?
        chunk = max(1, min(4096, (1 << 26) // N))
        steps = (N + chunk - 1) // chunk
        probe = min(4, steps)
        dense_counts(xy, cls, radii, chunk, first=1)                                                      # warm-up
        t_probe = events(lambda: dense_counts(xy, cls, radii, chunk, first=probe))[0]
        estimate = t_probe / probe * steps * 1e-3 * (opt.repeats + 1)
        run_dense = estimate <= opt.dense_budget
        if run_dense:
            assert torch.equal(dense_counts(xy, cls, radii, chunk), counts), 'the kernel and the dense tensor expressions differ'
        t_cells, t_nb, t_all, t_dense = [], [], [], []
        for _ in range(opt.repeats):
            t_cells.append(events(lambda: [ops.spatial_cells(pts, cell, ncx, ncy) for _ in range(INNER)])[0] / INNER)
            t_nb.append(events(lambda: [sorted_call() for _ in range(INNER)])[0] / INNER)
            t_all.append(events(lambda: ops.spatial_neighbors(xy, cls, C, radii))[0])
            if run_dense:
                t_dense.append(events(lambda: dense_counts(xy, cls, radii, chunk))[0])
        dense = stats(t_dense) if run_dense else f'not run (est. {estimate:.0f} s > {opt.dense_budget:g} s)'
        ratio = f'{med(t_dense) / med(t_all):18.1f}x' if run_dense else f'{"-":>19s}'
        lines.append(f'{N:8d} {side:8d} {ncx:5d}x{ncy:<5d} {float(counts[:, -1].sum()) / N:12.2f}  {stats(t_cells):>34s}  {stats(t_nb):>34s}  {stats(t_all):>34s}  '
                     f'{dense:>34s}  {ratio}')
        del pts, cell_start, counts, d2, row, again
        torch.cuda.empty_cache()
    text = '\n'.join(lines)
    print(text)
    if opt.out:
        with open(opt.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
