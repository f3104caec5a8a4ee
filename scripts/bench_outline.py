"""Outlines and hulls on the MI355X (csrc/outline.hip), measured: the three launches alone (hdy_label_outline_count, hdy_label_outline_write,
hdy_label_hull into buffers made beforehand) and the whole ops calls (ops.label_outline with its prefix sum and its read-back of the vertex
total, ops.label_hull) on the label map of a synthetic slide of 10^4 .. 2.5 x 10^5 nuclei, alternating with hdy_label_measure on the same map
(the bandwidth yardstick: one streaming pass over the same map bytes), and against the way out of the label map that exists without them: a
host loop over scipy.ndimage.find_objects with the Python restatement of tests/outline_ref.py per label.

    python scripts/bench_outline.py [--out profiles/outline_ab.txt] [--repeats 7] [--sizes 10000 100000 250000] [--host-labels 200]

Slides at nucleus density (bench_paste.py's: one object per 40 x 40 px), pasted into one int32 label map with elliptic 28 x 28 patches.
Device time between events for the launches and for ops.label_hull; ops.label_outline ends in a read-back, so it is timed by the host clock
around a synchronise.  The candidates alternate inside every repeat.  The host loop is timed on the first --host-labels labels that own pixels
(find_objects on the whole downloaded map once, then outline and hull per label on its crop) and EXTRAPOLATED to all labels: the column says so.
Before anything is timed the device results of those labels are checked equal to the restatement's."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import outline_ref  # noqa: E402
from bench_paste import events, slide_case, stats, wall  # noqa: E402
from hd_yolo_amd import _ext, ops  # noqa: E402


def host_loop(lm_host, R, rows):
    """(seconds of find_objects on the whole map, seconds of the per-label restatement over `rows`, their results)"""
    from scipy import ndimage
    t0 = time.perf_counter()
    slices = ndimage.find_objects(np.where((lm_host >= 0) & (lm_host < R), lm_host + 1, 0))
    t_find = time.perf_counter() - t0
    out = []
    t0 = time.perf_counter()
    for r in rows:
        sl = slices[r]
        y0, x0 = sl[0].start, sl[1].start
        crop = lm_host[sl]
        ext = [0, 0, crop.shape[1] - 1, crop.shape[0] - 1]
        v, area2, L, flag = outline_ref.outline(crop, r, ext)
        hi, hf = outline_ref.hull(crop, r, ext)
        out.append((v + [x0, y0], area2, L, hi, hf))
    return t_find, time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='')
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--sizes', type=int, nargs='*', default=[10000, 100000, 250000])
    ap.add_argument('--host-labels', type=int, default=200)
    opt = ap.parse_args()
    dev = torch.device('cuda', 0)
    med = statistics.median
    lines = ['command: python ' + ' '.join(sys.argv),
             f'device: {torch.cuda.get_device_name(0)}; ms, median [min .. max] over {opt.repeats} repeats; launches and ops.label_hull: device time between '
             'events; ops.label_outline: host clock around a synchronise (it reads the vertex total back); x = time over the label_measure yardstick',
             f'host loop: scipy find_objects on the whole map + tests/outline_ref.py per label, timed on {opt.host_labels} labels and EXTRAPOLATED to all', '']
    lines.append(f'{"labels":>8s} {"canvas":>7s} {"vertices":>9s} {"cracks":>9s}  {"label_measure (yardstick)":>34s}  {"outline_count launch":>34s} {"x":>6s}  '
                 f'{"outline_write launch":>34s} {"x":>6s}  {"hull launch":>34s} {"x":>6s}  {"ops.label_outline (wall)":>34s}  {"ops.label_hull":>34s}  '
                 f'{"host loop, extrapolated":>24s}  {"device speed-up":>15s}')
    for n in opt.sizes:
        boxes, masks, side = slide_case(n, dev)
        R = len(boxes)
        lm = ops.paste_label_map(masks, boxes, (side, side))
        del masks
        sums, extent = ops.label_measure(lm, R)
        offsets, verts, counts = ops.label_outline(lm, R, extent)
        hull_i, hull_f = ops.label_hull(lm, R, extent)
        assert not bool((counts[:, 3] & 6).any()) and not bool((hull_i[:, 3] & 6).any()), 'a label of the synthetic slide was flagged'
        # the host loop on a subsample, and its results against the device's
        lm_host = lm.cpu().numpy()
        rows = torch.nonzero(sums[:, 0] > 0)[:opt.host_labels, 0].tolist()
        t_find, t_rows, host = host_loop(lm_host, R, rows)
        off_h, verts_h, counts_h, hi_h, hf_h = (t.cpu().numpy() for t in (offsets, verts, counts, hull_i, hull_f))
        for r, (v, area2, L, hi, hf) in zip(rows, host):
            assert np.array_equal(verts_h[off_h[r]:off_h[r + 1]], v) and counts_h[r].tolist() == [len(v), area2, L, 0], r
            assert hi_h[r].tolist() == list(hi) and np.allclose(hf_h[r], hf, rtol=1e-9, atol=0), r
        owners = int((sums[:, 0] > 0).sum())
        t_host = t_find + t_rows / max(len(rows), 1) * owners
        del lm_host
        # the launches alone, into buffers made beforehand
        head = (lm.data_ptr(), lm.numel(), side, side, extent.data_ptr(), extent.numel(), R)
        c2, v2, st = torch.empty_like(counts), torch.empty_like(verts), torch.empty((1,), dtype=torch.int32, device=dev)
        hi2, hf2 = torch.empty_like(hull_i), torch.empty_like(hull_f)
        stream = ops.stream_ptr()
        launch_count = lambda: _ext.call('hdy_label_outline_count', *head, c2.data_ptr(), c2.numel(), stream)                          # noqa: E731
        launch_write = lambda: _ext.call('hdy_label_outline_write', *head, offsets.data_ptr(), offsets.numel(), v2.data_ptr(), v2.numel(),   # noqa: E731
                                         st.data_ptr(), stream)
        launch_hull = lambda: _ext.call('hdy_label_hull', *head, hi2.data_ptr(), hi2.numel(), hf2.data_ptr(), hf2.numel(), stream)     # noqa: E731
        for fn in (launch_count, launch_write, launch_hull):
            fn()
        assert torch.equal(c2, counts) and torch.equal(v2, verts) and int(st) == 0 and torch.equal(hi2, hull_i) and torch.equal(hf2, hull_f)
        t = {k: [] for k in ('measure', 'count', 'write', 'hull', 'ops_outline', 'ops_hull')}
        for _ in range(opt.repeats):
            t['measure'].append(events(lambda: ops.label_measure(lm, R))[0])
            t['count'].append(events(launch_count)[0])
            t['measure'].append(events(lambda: ops.label_measure(lm, R))[0])
            t['write'].append(events(launch_write)[0])
            t['measure'].append(events(lambda: ops.label_measure(lm, R))[0])
            t['hull'].append(events(launch_hull)[0])
            t['ops_outline'].append(wall(lambda: ops.label_outline(lm, R, extent))[0])
            t['ops_hull'].append(events(lambda: ops.label_hull(lm, R, extent))[0])
        y = med(t['measure'])
        dev_ms = med(t['ops_outline']) + med(t['ops_hull'])
        lines.append(f'{R:8d} {side:7d} {len(verts):9d} {int(counts[:, 2].sum()):9d}  {stats(t["measure"]):>34s}  {stats(t["count"]):>34s} {med(t["count"]) / y:5.2f}x  '
                     f'{stats(t["write"]):>34s} {med(t["write"]) / y:5.2f}x  {stats(t["hull"]):>34s} {med(t["hull"]) / y:5.2f}x  {stats(t["ops_outline"]):>34s}  '
                     f'{stats(t["ops_hull"]):>34s}  {t_host * 1e3:21.0f} ms  {t_host * 1e3 / dev_ms:14.0f}x')
        del lm
        torch.cuda.empty_cache()
    text = '\n'.join(lines)
    print(text)
    if opt.out:
        with open(opt.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
