"""Detection scoring on the MI355X: the host APMeter against the device path (csrc/score.hip), measured.

    python scripts/bench_score.py [--out profiles/score_ab.txt] [--repeats 7] [--batches 3] [--sizes 10000 100000 1000000] [--host-max 20000]

(a) val_nuclei.run on yolov5s (synthetic weights, SyntheticTiles, B = 64, 640 x 640, bf16): the `metrics` ms / image of the loop with the host
    meter (the code path of every earlier revision, still the default) and with DeviceAPMeter, beside `infer+nms` ms / image of the same run.
    The two modes alternate in one process after a warm-up run of each; run() brackets its three phases with device synchronisations.
    The end-of-epoch ap_per_class (identical curve arithmetic in both) is timed separately around summarize_stats.
(b) evaluation.score_slide on synthetic slide sets (synth.synth_slide_truth at nucleus density) of about 10^4, 10^5 and 10^6 detections: wall
    time of the whole call between device synchronisations (two device sorts, the match, one copy of the flags, the host curves), the device
    time of ops.ap_match alone on the ordered inputs (device events), the visited / total chunk-pair ratio, and the host APMeter (add +
    ap_per_class, a dense IoU matrix) at the sizes up to --host-max detections, where that matrix still fits in memory.
For each comparison the last column says whether the device path's slowest repeat beats the host path's fastest: the rule a later flip of
val_nuclei's default will use (the convention of NMS_GRID_MIN in hd_yolo_amd/ops.py)."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import evaluation  # noqa: E402
import val_nuclei  # noqa: E402
from hd_yolo_amd import ops, synth  # noqa: E402
from metayolo.datasets import SyntheticTiles  # noqa: E402
from metayolo.models.metrics import APMeter  # noqa: E402
from metayolo.models.yolo import Model  # noqa: E402


def stats(v):
    return f'{statistics.median(v):9.3f} [{min(v):9.3f} .. {max(v):9.3f}]'


def verdict(new, old):
    return '-' if not old else ('yes' if max(new) < min(old) else 'no')


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


def part_a(opt, dev, lines):
    nc, B, S = 8, 64, 640
    model = Model(synth.make_cfg('s', nc), synth.make_hyp())
    model.load_state_dict(synth.synth_state_dict(synth.shapes_of(model), seed=0), strict=False)
    model = model.to(dev)
    # summarize_stats is the end-of-epoch half (ap_per_class): timed on its own, outside run()'s `metrics` column
    tail, inner = [], val_nuclei.summarize_stats

    def timed_summary(meter, **kw):
        t0 = time.perf_counter()
        r = inner(meter, **kw)
        tail.append((time.perf_counter() - t0) * 1e3)
        return r

    val_nuclei.summarize_stats = timed_summary
    res = {False: [], True: []}
    fitness = {}
    try:
        for rep in range(opt.repeats + 1):                          # repeat 0 of each mode = warm-up (plans, allocator)
            for mode in (False, True):
                tail.clear()
                fit, _, speeds = val_nuclei.run(model, SyntheticTiles(B, S, nc, opt.batches, seed=12345), half=True, device_metrics=mode)
                fitness[mode] = fit
                if rep:
                    res[mode].append((speeds[1], speeds[2], sum(tail)))
    finally:
        val_nuclei.summarize_stats = inner
    assert fitness[False] == fitness[True], fitness
    lines.append(f'(a) val_nuclei.run, yolov5s, B = {B}, {S} x {S}, bf16, {opt.batches} batches per run, fitness {fitness[True]:.6f} in both modes; ms per image')
    lines.append(f'{"meter":8s}  {"metrics":>34s}  {"infer+nms (same runs)":>34s}  {"ap_per_class, ms per epoch":>34s}')
    for mode, name in ((False, 'host'), (True, 'device')):
        lines.append(f'{name:8s}  {stats([r[1] for r in res[mode]]):>34s}  {stats([r[0] for r in res[mode]]):>34s}  {stats([r[2] for r in res[mode]]):>34s}')
    lines.append(f'device metrics max < host metrics min: {verdict([r[1] for r in res[True]], [r[1] for r in res[False]])}')
    lines.append('')


def part_b(opt, dev, lines):
    lines.append('(b) evaluation.score_slide on synth.synth_slide_truth sets (4 classes, 40 x 40 px per object); ms')
    lines.append(f'{"detections":>10s} {"truths":>8s} {"mAP@.5":>7s} {"visited/total chunk pairs":>28s}  {"score_slide, whole call":>34s}  {"ap_match alone":>34s}  '
                 f'{"host APMeter add + ap_per_class":>34s}  device max < host min')
    for n in opt.sizes:
        n_obj = max(int(n / 1.112), 1)
        tb, tl, pb, ps, pl = (torch.from_numpy(a).to(dev) for a in synth.synth_slide_truth(n_obj, 40.0 * n_obj ** 0.5, 4, seed=1))
        result, truth = {'boxes': pb, 'scores': ps, 'labels': pl}, {'boxes': tb, 'labels': tl}
        info = {}
        st = evaluation.score_slide(result, truth, info=info)       # warm-up
        op, ot = evaluation.slide_orders(pb, tb)
        off = lambda k: torch.tensor([0, k], dtype=torch.int32, device=dev)   # noqa: E731
        args = (pb[op], ps[op], pl[op], off(len(ps)), tb[ot], tl[ot], off(len(tl)), torch.linspace(0.5, 0.95, 10))
        rows = dict(pred_row=op.to(torch.int32), true_row=ot.to(torch.int32))
        ops.ap_match(*args, **rows)

        def host():
            m = APMeter()
            m.add(result, truth)
            return m.ap_per_class(iouv=torch.linspace(0.5, 0.95, 10), ignore=[-100, -1])

        run_host = len(ps) <= opt.host_max
        t_all, t_match, t_host = [], [], []
        for _ in range(opt.repeats):
            if run_host:
                t, hs = wall(host)
                t_host.append(t)
            t_all.append(wall(lambda: evaluation.score_slide(result, truth))[0])
            t_match.append(events(lambda: ops.ap_match(*args, **rows))[0])
        if run_host:
            assert abs(float(hs['ap'][:, 0].mean()) - float(st['ap'][:, 0].mean())) < 1e-12
        ratio = f'{info["chunks_visited"]} / {info["chunks_total"]} = {info["chunks_visited"] / max(info["chunks_total"], 1):.4f}'
        host_txt = stats(t_host) if t_host else 'not run (dense IoU matrix)'
        lines.append(f'{len(ps):10d} {len(tl):8d} {float(st["ap"][:, 0].mean()):7.4f} {ratio:>28s}  {stats(t_all):>34s}  {stats(t_match):>34s}  {host_txt:>34s}  '
                     f'{verdict(t_all, t_host)}')
    lines.append('')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='')
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--batches', type=int, default=3)
    ap.add_argument('--sizes', type=int, nargs='*', default=[10000, 100000, 1000000])
    ap.add_argument('--host-max', type=int, default=20000, help='largest detection count the host APMeter is run at (its IoU matrix is dense)')
    ap.add_argument('--skip-a', action='store_true')
    opt = ap.parse_args()
    dev = torch.device('cuda', 0)
    lines = ['command: python ' + ' '.join(sys.argv), f'device: {torch.cuda.get_device_name(0)}; median [min .. max] over {opt.repeats} alternated repeats', '']
    if not opt.skip_a:
        part_a(opt, dev, lines)
    part_b(opt, dev, lines)
    text = '\n'.join(lines)
    print(text)
    if opt.out:
        with open(opt.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
