"""Whole-slide merge on the MI355X: where the time goes, and the A/B of the two explicit-box NMS paths.

    python scripts/bench_slide.py --ab [--out profiles/nms_grid_ab.txt]      one-workgroup kernel (ops._nms_launch) vs ops.nms_grid
    python scripts/bench_slide.py --slide 20000 [--grid-min 0]                synthetic slide -> evaluation.inference_on_slide
    python scripts/bench_slide.py --slide 20000 --u8 [--min-tissue 0.05]      the same from a synthetic 8-bit (H, W, 3) slide (tile gather + device merge)
    python scripts/bench_slide.py --slide-ab 8000 20000 [--out profiles/slide_u8_ab.txt]   float path vs 8-bit path on the same pixels
    python scripts/bench_slide.py --masks-ab 2560 5120 [--out profiles/slide_masks_ab.txt]   masks of an 8-bit slide: device mask rows vs HDY_DEVICE_MASKS=0
    python scripts/bench_slide.py --once 262144                               one nms_grid call (for a kernel trace of its own)

--masks-ab: the synthetic mask model of `evaluation.py --masks` (tiny variant, one mask class, fp32, conf_thres 0.05) on a synthetic 8-bit slide
per size; evaluation.inference_on_slide(..., compute_masks=True, label_map=True) with the device mask rows (Detect.masks_device, the masks
beside the device append) against HDY_DEVICE_MASKS=0 (Detect.attach_masks per batch and the Python merge: the path before the switch
existed), alternating in one process after a warm-up of each side that builds the plans.  Wall time around each call between device
synchronisations; the results of the two sides are compared with torch.equal before anything is timed.

--slide-ab: per size one random 8-bit slide on the device and three ways through evaluation.inference_on_slide, alternating, after a warm-up of
each: "float" = the float path fed table[v] as float CHW already on the device (its best case), "convert + float" = the same with the
conversion a caller of the float path needs (8-bit HWC -> float CHW on the device) inside the timed region, "8-bit" = the slide as it is.
Wall time around each call between device synchronisations; merge NMS timed inside by two more synchronisations (all sides alike);
peak device memory per side = the slide it reads + the call's own peak (torch.cuda.max_memory_allocated above the resident set).

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


def _slide_setup(opt):
    """(evaluation module, deployed yolov5 on the device, merge-NMS stopwatch)"""
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
    return evaluation, deployed, merge, dev


def u8_slide(S, dev, seed=5):
    """synthetic 8-bit slide (S, S, 3) from a seed, made on the device"""
    return torch.randint(0, 256, (S, S, 3), dtype=torch.uint8, device=dev, generator=torch.Generator(device=dev).manual_seed(seed))


def float_of(u8):
    """table[v] as float CHW, table = arange(256) / 255 made on the CPU (the 8-bit path's pixel values, bit for bit), in row strips"""
    table = (torch.arange(256).float() / 255).to(u8.device)
    out = torch.empty((3,) + tuple(u8.shape[:2]), dtype=torch.float32, device=u8.device)
    for r in range(0, u8.shape[0], 1024):
        out[:, r:r + 1024] = table[u8[r:r + 1024, :, :3].long()].permute(2, 0, 1)
    return out


def slide_ab(opt):
    evaluation, deployed, merge, dev = _slide_setup(opt)
    kw = dict(tile=opt.tile, overlap=opt.overlap, batch_size=opt.batch_size)
    lines = ['command: python ' + ' '.join(sys.argv),
             f'device: {torch.cuda.get_device_name(0)}; yolov5{opt.variant}, tile {opt.tile}, overlap {opt.overlap}, batch {opt.batch_size}; times in ms, '
             f'median [min .. max] over {opt.repeats} repeats, sides alternating; peak = the slide a side reads + what the call allocates on top (torch.cuda.max_memory_allocated), MB']
    for S in opt.slide_ab:
        u8 = u8_slide(S, dev)
        flt = float_of(u8)
        sides = {
            'float CHW on device (old)': lambda: evaluation.inference_on_slide(deployed, flt, **kw),
            'convert + float (old)': lambda: evaluation.inference_on_slide(deployed, u8.permute(2, 0, 1).float().div_(255), **kw),
            '8-bit HWC (new)': lambda: evaluation.inference_on_slide(deployed, u8, **kw),
        }
        rec = {k: {'net': [], 'merge': [], 'total': [], 'peak': 0, 'kept': 0} for k in sides}
        for fn in sides.values():
            fn()                                                          # plans, allocator
        for _ in range(opt.repeats):
            for k, fn in sides.items():
                merge.update(ms=0.0, boxes=0)
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                t0 = time.time()
                out = fn()
                torch.cuda.synchronize()
                total = (time.time() - t0) * 1e3
                r = rec[k]
                r['net'].append(total - merge['ms'])
                r['merge'].append(merge['ms'])
                r['total'].append(total)
                reads = flt if k.startswith('float') else u8             # both slides are resident throughout: count the one this side reads
                r['peak'] = max(r['peak'], (torch.cuda.max_memory_allocated() - base + reads.numel() * reads.element_size()) >> 20)
                r['kept'] = sum(len(v['boxes']) for v in out.values())
                del out
        tiles = len(evaluation.slide_rois(S, S, opt.tile, opt.overlap))
        lines.append(f'slide {S} x {S}: {tiles} tiles')
        lines.append(f'  {"side":28s} {"network + tiling":>34s}  {"merge NMS":>34s}  {"total":>34s}  {"peak MB":>8s}  {"kept":>8s}')
        for k, r in rec.items():
            lines.append(f'  {k:28s} {stats(r["net"]):>34s}  {stats(r["merge"]):>34s}  {stats(r["total"]):>34s}  {r["peak"]:8d}  {r["kept"]:8d}')
        new, old, conv = rec['8-bit HWC (new)'], rec['float CHW on device (old)'], rec['convert + float (old)']
        lines.append(f'  new slowest total < old fastest total: {"yes" if max(new["total"]) < min(old["total"]) else "no"}'
                     f' (float on device), {"yes" if max(new["total"]) < min(conv["total"]) else "no"} (convert + float)')
        print('\n'.join(lines[-6:]), flush=True)
        del u8, flt, sides
        torch.cuda.empty_cache()
    text = '\n'.join(lines) + '\n'
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, 'w') as f:
            f.write(text)
    print(text)


def masks_ab(opt):
    import evaluation
    from metayolo.models.yolo import Deploy, Model
    dev = torch.device('cuda', 0)
    cfg = synth.make_cfg('n', 2)
    cfg['headers'][0][3][3] = 1                                           # one mask class: the mask model of evaluation.py --masks
    mm = Model(cfg, synth.make_hyp(conf_thres=0.05))
    mm.load_state_dict(synth.mask_state_dict(mm), strict=False)
    dep = Deploy(mm.to(dev).eval())
    lines = ['command: python ' + ' '.join(sys.argv),
             f'device: {torch.cuda.get_device_name(0)}; mask model (yolov5n, one mask class, fp32), tile {opt.tile}, overlap {opt.overlap}, batch {opt.batch_size}, '
             f'compute_masks + label_map; times in ms, median [min .. max] over {opt.repeats} repeats, sides alternating',
             f'{"slide":>7s} {"tiles":>6s} {"batches":>7s} {"kept":>8s}  {"side":24s} {"ms / slide":>34s}  {"ms / batch (median)":>20s}']
    sides = {'HDY_DEVICE_MASKS=0 (old)': '0', 'device mask rows (new)': '1'}
    verdicts = []
    for S in opt.masks_ab:
        slide = (synth.synth_images(1, S, seed=5)[0] * 255).round().to(torch.uint8).permute(1, 2, 0).contiguous().to(dev)
        kw = dict(tile=min(opt.tile, S), overlap=opt.overlap, batch_size=opt.batch_size, compute_masks=True, label_map=True)

        def run(flag):
            os.environ['HDY_DEVICE_MASKS'] = flag
            return evaluation.inference_on_slide(dep, slide, **kw)

        first = {k: run(flag) for k, flag in sides.items()}               # plans, packings, allocator
        old, new = (first[k]['det'] for k in sides)
        assert sorted(old) == sorted(new) and all(torch.equal(old[k], new[k]) for k in old), 'the two sides differ'
        kept = len(new['boxes'])
        del first, old, new
        rec = {k: [] for k in sides}
        for _ in range(opt.repeats):
            for k, flag in sides.items():
                torch.cuda.synchronize()
                t0 = time.time()
                out = run(flag)
                torch.cuda.synchronize()
                rec[k].append((time.time() - t0) * 1e3)
                del out
        tiles = len(evaluation.slide_rois(S, S, kw['tile'], opt.overlap))
        batches = -(-tiles // opt.batch_size)
        for k, v in rec.items():
            lines.append(f'{S:7d} {tiles:6d} {batches:7d} {kept:8d}  {k:24s} {stats(v):>34s}  {statistics.median(v) / batches:20.3f}')
        o, n = rec['HDY_DEVICE_MASKS=0 (old)'], rec['device mask rows (new)']
        verdicts.append(statistics.median(n) <= statistics.median(o))
        lines.append(f'{"":7s} new median <= old median: {"yes" if verdicts[-1] else "no"}; new slowest < old fastest: {"yes" if max(n) < min(o) else "no"}')
        print('\n'.join(lines[-3:]), flush=True)
        del slide
        torch.cuda.empty_cache()
    os.environ.pop('HDY_DEVICE_MASKS', None)
    text = '\n'.join(lines) + '\n'
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, 'w') as f:
            f.write(text)
    print(text)


def slide(opt):
    evaluation, deployed, merge, dev = _slide_setup(opt)
    S = opt.slide
    extra = {}
    if opt.u8:
        img = u8_slide(S, dev)
        warm = img[:min(S, 1280), :min(S, 1280)].contiguous()
        extra = dict(min_tissue=opt.min_tissue)
    else:
        img = torch.rand((3, S, S), device=dev, generator=torch.Generator(device=dev).manual_seed(5))
        warm = img[:, :min(S, 1280), :min(S, 1280)].contiguous()
    evaluation.inference_on_slide(deployed, warm, tile=opt.tile, overlap=opt.overlap, batch_size=opt.batch_size, **extra)        # plans, allocator
    merge.update(ms=0.0, boxes=0)
    torch.cuda.synchronize()
    t0 = time.time()
    torch.cuda.reset_peak_memory_stats()
    out = evaluation.inference_on_slide(deployed, img, tile=opt.tile, overlap=opt.overlap, batch_size=opt.batch_size, **extra)
    torch.cuda.synchronize()
    total = (time.time() - t0) * 1e3
    tiles = len(evaluation.slide_rois(S, S, opt.tile, opt.overlap))
    kept = sum(len(v['boxes']) for v in out.values())
    print(f'slide {S}x{S}{" 8-bit" if opt.u8 else ""}: {tiles} tiles, peak {torch.cuda.max_memory_allocated() >> 20} MB, HDY_NMS_GRID_MIN={os.environ.get("HDY_NMS_GRID_MIN", "default " + str(ops.NMS_GRID_MIN))}, '
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
    ap.add_argument('--u8', action='store_true', help='--slide: a synthetic 8-bit (S, S, 3) slide from the seed, through the tile gather and the device merge')
    ap.add_argument('--min-tissue', type=float, default=0.0, help='--slide --u8: skip tiles with less than this fraction of non-background pixels')
    ap.add_argument('--slide-ab', type=int, nargs='*', default=[], help='sizes for the float path vs 8-bit path comparison')
    ap.add_argument('--masks-ab', type=int, nargs='*', default=[], help='sizes for the device mask rows vs HDY_DEVICE_MASKS=0 comparison on 8-bit slides')
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
    if opt.slide_ab:
        slide_ab(opt)
    if opt.masks_ab:
        masks_ab(opt)
    if opt.slide:
        slide(opt)
    if opt.once:
        once(opt)
