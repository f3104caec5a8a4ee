"""The cell graph on the MI355X (csrc/graph.hip), measured: hdy_graph_knn alone, hdy_graph_mutual alone and the whole ops.spatial_knn call (cell
ids, the stable device sort, packing, hdy_spatial_cells and hdy_graph_knn) at k = 8 within 128 px on synthetic slides of 10^4 .. 2.5 x 10^5
nuclei, against the same neighbours from a chunked torch.cdist + topk on the same device (a chunk x N float64 distance block per step).

    python scripts/bench_graph.py [--out profiles/graph_ab.txt] [--repeats 5] [--sizes 10000 100000 250000] [--dense-budget 30]

Slides at nucleus density (one nucleus per 40 x 40 px): uniform positions, and one clustered set (70 % of the nuclei in Gaussian clusters of 30 px,
the rest uniform) at the middle size.  The yardstick runs in the same process and alternates with the kernel inside every repeat; its first
chunks are timed and the run is made only where the extrapolated time of all its repeats stays within --dense-budget seconds ("not run"
otherwise).  Where it runs, its distances are checked against the kernel's before anything is timed (the kernel's own answer is held to a
brute-force integer restatement by tests/test_gpu_graph.py); a yardstick that disagrees is reported and not timed.  Device time between events; the two
kernels alone are timed as INNER back-to-back calls per repeat and reported per call.

The second table sweeps the default cell size of ops.spatial_knn: the cell that holds fill * k points (ops.KNN_CELL_FILL = the x1 column)
at x1/2, x1, x2 and x4 of that fill, the kernel alone and the whole call, the four alternated inside every repeat."""
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
from hd_yolo_amd import ops, spatial  # noqa: E402

K = 8
MAX_PX = 128
INNER = 20          # back-to-back calls per timed window of a kernel alone
FACTORS = (0.5, 1.0, 2.0, 4.0)


def points(n, kind, dev, seed=1):
    """(xy int32 (n, 2) units on the device, side in px)"""
    side = int(math.ceil(40.0 * n ** 0.5))
    g = torch.Generator().manual_seed(seed)
    px = torch.rand((n, 2), generator=g, dtype=torch.float64) * side
    if kind == 'clustered':
        centres = torch.rand((max(n // 500, 1), 2), generator=g, dtype=torch.float64) * side
        pick = torch.randint(0, len(centres), (n,), generator=g)
        near = centres[pick] + torch.randn((n, 2), generator=g, dtype=torch.float64) * 30.0
        px = torch.where((torch.rand((n, 1), generator=g) < 0.7), near, px).clamp(0, side - 1e-3)
    return spatial.to_units(px.to(dev)), side


def dense_knn(xy, k, r, chunk, first=None):
    """(dist float64 (N, k) in units, inf padding; rows int64 (N, k)) by torch.cdist and topk, a chunk of queries per step"""
    N = xy.shape[0]
    p = xy.double()
    dist = torch.full((N, k), float('inf'), dtype=torch.float64, device=xy.device)
    rows = torch.full((N, k), -1, dtype=torch.int64, device=xy.device)
    for n, q0 in enumerate(range(0, N, chunk)):
        if first is not None and n >= first:
            break
        q1 = min(q0 + chunk, N)
        d = torch.cdist(p[q0:q1], p, compute_mode='donot_use_mm_for_euclid_dist')
        d[torch.arange(q1 - q0, device=xy.device), torch.arange(q0, q1, device=xy.device)] = float('inf')      # a point is not its own neighbour
        v, i = torch.topk(d, min(k, N), dim=1, largest=False)
        beyond = v > r
        dist[q0:q1, :v.shape[1]] = torch.where(beyond, float('inf'), v)
        rows[q0:q1, :v.shape[1]] = torch.where(beyond, -1, i)
    return dist, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--sizes', type=int, nargs='*', default=[10000, 100000, 250000])
    ap.add_argument('--dense-budget', type=float, default=30.0, help='seconds all repeats of the dense yardstick may take at one set')
    opt = ap.parse_args()
    dev = torch.device('cuda', 0)
    r = spatial.radius_units(MAX_PX)
    lines = ['command: python ' + ' '.join(sys.argv),
             f'device: {torch.cuda.get_device_name(0)}; device ms between events, median [min .. max] over {opt.repeats} repeats; k = {K} within {MAX_PX} px',
             f'hdy_graph_knn / hdy_graph_mutual: per call, {INNER} back-to-back calls per window (host issue time included)', '']
    head = (f'{"nuclei":>8s} {"set":>9s} {"side px":>8s} {"cells":>11s} {"mean nb":>8s}  {"hdy_graph_knn":>34s}  {"hdy_graph_mutual":>34s}  '
            f'{"ops.spatial_knn (whole call)":>34s}  {"cdist + topk":>34s}  {"whole call vs dense":>19s}')
    lines.append(head)
    sweep = ['', f'default cell size: the cell that holds fill * k points, fill = {ops.KNN_CELL_FILL} x factor; per factor the kernel alone / the whole call',
             f'{"nuclei":>8s} {"set":>9s}  ' + '  '.join(f'{"x" + format(f, "g") + " cells, hdy_graph_knn, ops.spatial_knn":>48s}' for f in FACTORS)]
    med = statistics.median
    sets = [(n, 'uniform') for n in opt.sizes]
    if len(opt.sizes) > 1:
        sets.insert(2, (opt.sizes[1], 'clustered'))
    for n, kind in sets:
        xy, side = points(n, kind, dev)
        N = xy.shape[0]
        extent = (side * spatial.UNITS, side * spatial.UNITS)
        info = {}
        row, d2, count = ops.spatial_knn(xy, K, r, extent_units=extent, info=info)
        assert int(info['status']) == 0
        pts, cell_start, cell, ncx, ncy = (info[k] for k in ('pts', 'cell_start', 'cell_units', 'ncx', 'ncy'))
        sorted_call = lambda: ops.spatial_knn_sorted(pts, cell_start, cell, ncx, ncy, K, r)               # noqa: E731
        assert all(torch.equal(a, b) for a, b in zip(sorted_call(), (row, d2, count)))
        # the yardstick: is it affordable here?
        chunk = max(1, min(1024, (1 << 24) // N))            # torch.cdist's direct form returned wrong rows for a 4096 x 10^4 block on this device; 2^24 entries are safe
        steps = (N + chunk - 1) // chunk
        probe = min(4, steps)
        dense_knn(xy, K, r, chunk, first=1)                                                               # warm-up
        t_probe = events(lambda: dense_knn(xy, K, r, chunk, first=probe))[0]
        estimate = t_probe / probe * steps * 1e-3 * (opt.repeats + 1)
        run_dense = estimate <= opt.dense_budget
        differs = ''
        if run_dense:
            dist, _ = dense_knn(xy, K, r, chunk)
            mine = torch.where(d2 < 0, float('inf'), torch.sqrt(d2.double()))
            if not torch.equal(torch.isinf(dist), torch.isinf(mine)):
                differs = 'other numbers of neighbours than the kernel'
            elif not torch.allclose(torch.nan_to_num(dist, posinf=0.0), torch.nan_to_num(mine, posinf=0.0), rtol=1e-9, atol=1e-6):
                differs = 'other distances than the kernel'
            run_dense = not differs                                # a yardstick that is wrong is not timed
        t_knn, t_mut, t_all, t_dense = [], [], [], []
        for _ in range(opt.repeats):
            t_knn.append(events(lambda: [sorted_call() for _ in range(INNER)])[0] / INNER)
            t_mut.append(events(lambda: [ops.knn_mutual(row) for _ in range(INNER)])[0] / INNER)
            t_all.append(events(lambda: ops.spatial_knn(xy, K, r, extent_units=extent))[0])
            if run_dense:
                t_dense.append(events(lambda: dense_knn(xy, K, r, chunk))[0])
        dense = stats(t_dense) if run_dense else f'not run ({differs})' if differs else f'not run (est. {estimate:.0f} s > {opt.dense_budget:g} s)'
        ratio = f'{med(t_dense) / med(t_all):18.1f}x' if run_dense else f'{"-":>19s}'
        lines.append(f'{N:8d} {kind:>9s} {side:8d} {ncx:5d}x{ncy:<5d} {float(count.sum()) / N:8.2f}  {stats(t_knn):>34s}  {stats(t_mut):>34s}  {stats(t_all):>34s}  '
                     f'{dense:>34s}  {ratio}')
        # the sweep of the default cell size
        forms = []
        for f in FACTORS:
            c = ops.knn_cell_units(N, K, r, extent[0] - 1, extent[1] - 1, fill=ops.KNN_CELL_FILL * f)
            i = {}
            got = ops.spatial_knn(xy, K, r, cell_units=c, extent_units=extent, info=i)
            assert all(torch.equal(a, b) for a, b in zip(got, (row, d2, count))), 'the result depends on the cell size'
            forms.append((c, i))
        t_k, t_a = [[] for _ in FACTORS], [[] for _ in FACTORS]
        for _ in range(opt.repeats):
            for j, (c, i) in enumerate(forms):
                t_k[j].append(events(lambda: [ops.spatial_knn_sorted(i['pts'], i['cell_start'], c, i['ncx'], i['ncy'], K, r) for _ in range(INNER)])[0] / INNER)
                t_a[j].append(events(lambda: ops.spatial_knn(xy, K, r, cell_units=c, extent_units=extent))[0])
        sweep.append(f'{N:8d} {kind:>9s}  ' + '  '.join(f'{i["ncx"]:4d}x{i["ncy"]:<4d} {med(t_k[j]):7.3f} [{min(t_k[j]):7.3f}..{max(t_k[j]):7.3f}] {med(t_a[j]):7.3f} [{min(t_a[j]):7.3f}..{max(t_a[j]):7.3f}]'
                                                        for j, (c, i) in enumerate(forms)))
        del pts, cell_start, row, d2, count, forms
        torch.cuda.empty_cache()
    text = '\n'.join(lines + sweep)
    print(text)
    if opt.out:
        with open(opt.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
