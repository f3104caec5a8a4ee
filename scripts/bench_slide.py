"""Whole-slide merge on the MI355X: where the time goes, and the A/B of the two explicit-box NMS paths.

    python scripts/bench_slide.py --ab [--out profiles/nms_grid_ab.txt]      one-workgroup kernel (ops._nms_launch) vs ops.nms_grid
    python scripts/bench_slide.py --slide 20000 [--grid-min 0]                synthetic slide -> evaluation.inference_on_slide
    python scripts/bench_slide.py --once 262144                               one nms_grid call (for a kernel trace of its own)

--ab: both paths on the same device tensors in one process, alternating, after a warm-up call of each; device events around each call (both
end in a synchronising read of the kept count); median and min-max over --repeats.  Sets: slide (objects of 12-30 px detected 1-3 times,
0.001 objects per px^2), dense (12-30 px boxes at 16 384 per 640 x 640 tile), packed (4-44 px boxes, all centres inside 300 x 300 px).  The old path is skipped above --old-max boxes (it is
O(M x kept) on one workgroup: 4.6 s at 250 k boxes) unless --old-once, which runs it a single time there."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from hd_yolo_amd import ops, synth  # noqa: E402

SLIDE_DENSITY = 16000 / 4000.0 ** 2         # objects per px^2 of the slide-like sets (tests use the same)


def slide_set(m, seed=1):
    n_obj = max(m // 2, 1)
    b, s = synth.synth_slide_boxes(n_obj, (n_obj / SLIDE_DENSITY) ** 0.5, seed)
    return b[:m], s[:m]


def packed_set(m, seed=1):
    """the densest sets of the test suite (tests/test_gpu_f3.py): boxes of 4-44 px with centres in 300 x 300 px, whatever their number"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(0, 300, (m, 2))
    wh = rng.uniform(4, 44, (m, 2))
    return np.concatenate([c - wh / 2, c + wh / 2], 1).astype(np.float32), rng.uniform(0, 1, m).astype(np.float32)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), r


def stats(v):
    return f'{statistics.median(v):9.3f} [{min(v):9.3f} .. {max(v):9.3f}]'


def ab(opt):
    dev = torch.device('cuda', 0)
    lines = ['command: python ' + ' '.join(sys.argv), f'device: {torch.cuda.get_device_name(0)}; times in ms, median [min .. max] over {opt.repeats} repeats',
             f'{"set":8s} {"M":>8s} {"thr":>5s} {"kept":>8s} {"rounds":>6s}  {"one workgroup (old)":>34s}  {"nms_grid (new)":>34s}  new max < old min']
    points = [('slide', m) for m in (2048, 4096, 8192, 16384, 32768, 65536, 131072, 262144, 1048576)] + [('dense', 4096), ('dense', 8192), ('dense', 16384)] + \
             [('packed', 4096), ('packed', 8192), ('packed', 16384)]
    for kind, m in points:
        b, s = slide_set(m) if kind == 'slide' else synth.synth_dense_boxes(m, 1) if kind == 'dense' else packed_set(m)
        bt, st = torch.from_numpy(b).to(dev), torch.from_numpy(s).to(dev)
        thr = 0.45
        info = {}
        new = lambda: ops.nms_grid(bt, st, thr, info=info)
        old = lambda: ops._nms_launch(bt, st, thr, len(b))
        run_old = len(b) <= opt.old_max
        r_new = new()
        t_old, t_new = [], []
        if run_old:
            assert torch.equal(old(), r_new)
        for _ in range(opt.repeats):
            if run_old:
                t_old.append(timed(old)[0])
            t_new.append(timed(new)[0])
        if not run_old and opt.old_once and len(b) <= opt.old_once_max:
            t, r = timed(old)
            assert torch.equal(r, r_new)
            t_old = [t]
        verdict = '-' if not t_old else ('yes' if max(t_new) < min(t_old) else 'no')
        old_txt = stats(t_old) if len(t_old) > 1 else (f'{t_old[0]:9.3f} (one run)' if t_old else 'not measured')
        lines.append(f'{kind:8s} {len(b):8d} {thr:5.2f} {len(r_new):8d} {info["rounds"]:6d}  {old_txt:>34s}  {stats(t_new):>34s}  {verdict}')
        print(lines[-1], flush=True)
    text = '\n'.join(lines) + '\n'
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, 'w') as f:
            f.write(text)
    print(text)


def slide(opt):
    import evaluation
    from metayolo.models.yolo import Model
    dev = torch.device('cuda', 0)
    if opt.grid_min is not None:
        os.environ['HDY_NMS_GRID_MIN'] = str(opt.grid_min)
    ref = Model(synth.make_cfg(opt.variant, opt.nc), synth.make_hyp())
    ref.load_state_dict(synth.synth_state_dict(synth.shapes_of(ref), seed=0), strict=False)
    model, deployed = evaluation.build_model(ref, half=True)
    deployed = deployed.to(dev)
    merge = {'ms': 0.0, 'boxes': 0}
    inner = evaluation.nms

    def timed_nms(boxes, scores, thr):
        torch.cuda.synchronize()
        t = time.time()
        r = inner(boxes, scores, thr)
        torch.cuda.synchronize()
        merge['ms'] += (time.time() - t) * 1e3
        merge['boxes'] += len(boxes)
        return r

    evaluation.nms = timed_nms
    S = opt.slide
    img = torch.rand((3, S, S), device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    warm = img[:, :min(S, 1280), :min(S, 1280)].contiguous()
    evaluation.inference_on_slide(deployed, warm, tile=opt.tile, overlap=opt.overlap, batch_size=opt.batch_size)        # plans, allocator
    merge.update(ms=0.0, boxes=0)
    torch.cuda.synchronize()
    t0 = time.time()
    out = evaluation.inference_on_slide(deployed, img, tile=opt.tile, overlap=opt.overlap, batch_size=opt.batch_size)
    torch.cuda.synchronize()
    total = (time.time() - t0) * 1e3
    tiles = len(evaluation.slide_rois(S, S, opt.tile, opt.overlap))
    kept = sum(len(v['boxes']) for v in out.values())
    print(f'slide {S}x{S}: {tiles} tiles, HDY_NMS_GRID_MIN={os.environ.get("HDY_NMS_GRID_MIN", "default " + str(ops.NMS_GRID_MIN))}, '
          f'{merge["boxes"]} merged boxes -> {kept} kept; network + tiling {total - merge["ms"]:.1f} ms, merge NMS {merge["ms"]:.1f} ms, total {total:.1f} ms')


def once(opt):
    dev = torch.device('cuda', 0)
    b, s = slide_set(opt.once)
    bt, st = torch.from_numpy(b).to(dev), torch.from_numpy(s).to(dev)
    info = {}
    for _ in range(2):
        r = ops.nms_grid(bt, st, 0.45, info=info)
    print(f'M={len(b)} kept={len(r)} {info}')


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--ab', action='store_true')
    ap.add_argument('--slide', type=int, default=0)
    ap.add_argument('--once', type=int, default=0)
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--old-max', type=int, default=140000, help='largest set the one-workgroup kernel is timed on repeatedly')
    ap.add_argument('--old-once', action='store_true', help='one run of the one-workgroup kernel above --old-max too')
    ap.add_argument('--old-once-max', type=int, default=300000, help='... but never above this (minutes of one workgroup on a shared card)')
    ap.add_argument('--out', default='')
    ap.add_argument('--grid-min', type=int, default=None)
    ap.add_argument('--variant', default='s')
    ap.add_argument('--nc', type=int, default=8)
    ap.add_argument('--tile', type=int, default=640)
    ap.add_argument('--overlap', type=int, default=64)
    ap.add_argument('--batch-size', type=int, default=32)
    opt = ap.parse_args()
    if opt.ab:
        ab(opt)
    if opt.slide:
        slide(opt)
    if opt.once:
        once(opt)
