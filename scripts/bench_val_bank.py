"""What validation costs per image on the two paths of val_nuclei.run, measured and not judged (no threshold):

  bank   BankTiles -> 8-bit forward (Model.forward_tiles), device metrics, masks scored (mask AP, PQ / AJI / Dice)
  float  the same tiles and truths as a plain list of float batches -> Model.forward, host APMeter, boxes only

on a synthetic bank (hd_yolo_amd.synth.synth_tile_bank with an instance map) and a stock graph with the mask branch and synthetic weights.
conf_thres is 0.001 so that the synthetic weights yield detections for the NMS, the mask head and the meters to work on (their number is
printed).  The two paths alternate, `--repeats` times each after one warm-up pass each; per path the median and the min .. max of run()'s
three `speeds` (pre / infer+nms / metrics, ms per image) are printed.

Usage: python scripts/bench_val_bank.py [--tiles 64] [--size 640] [--variant s] [--nc 8] [--batch 32] [--repeats 5] [--out profiles/val_bank.txt]"""
import argparse
import os
import statistics
import subprocess
import sys

os.environ.setdefault('YOLOv5_VERBOSE', 'false')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import val_nuclei  # noqa: E402
from hd_yolo_amd import synth  # noqa: E402
from metayolo.datasets import BankTiles  # noqa: E402
from metayolo.models.yolo import Model  # noqa: E402


def commit():
    try:
        return subprocess.run(['git', 'rev-parse', '--short', 'HEAD'], cwd=ROOT, capture_output=True, text=True, timeout=10).stdout.strip() or 'unknown'
    except (OSError, subprocess.SubprocessError):
        return 'unknown'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tiles', type=int, default=64)
    ap.add_argument('--size', type=int, default=640)
    ap.add_argument('--variant', default='s')
    ap.add_argument('--nc', type=int, default=8)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--commit', default='', help='recorded in the output (default: git rev-parse of the checkout)')
    ap.add_argument('--out', default='', help='also write the report to this file')
    opt = ap.parse_args()
    dev = torch.device('cuda', 0)
    cfg = synth.make_cfg(opt.variant, opt.nc)
    cfg['headers'][0][3][3] = 1                                         # the mask branch, one shared mask class
    model = Model(cfg, synth.make_hyp(conf_thres=0.001))
    model.load_state_dict(synth.synth_state_dict(synth.shapes_of(model), seed=0), strict=False)
    model = model.to(dev).eval()
    bank = synth.synth_tile_bank(opt.tiles, opt.size, opt.nc, instances=True)
    paths = {
        'bank': lambda: val_nuclei.run(model, BankTiles(bank, opt.batch, device=dev), half=True, device_metrics=True),
        'float': lambda: val_nuclei.run(model, float_batches, half=True, device_metrics=False),
    }
    float_batches = list(BankTiles(bank, opt.batch, device=dev, masks=False))
    speeds, last = {k: [] for k in paths}, {}
    for k, fn in paths.items():                                          # warm-up: plans, workspaces
        fn()
    for _ in range(max(opt.repeats, 1)):
        for k, fn in paths.items():
            fitness, stats, sp = fn()
            speeds[k].append(sp)
            last[k] = (fitness, stats)
    masks = last['bank'][1]['det']['masks']
    lines = [f'command: python scripts/bench_val_bank.py {" ".join(sys.argv[1:])}'.rstrip(), f'commit: {opt.commit or commit()}',
             f'device: {torch.cuda.get_device_name(0)}',
             f'workload: {opt.tiles} tiles of {opt.size} x {opt.size}, {len(bank.labels)} truths, yolov5{opt.variant} nc={opt.nc} + mask branch, bf16, batch {opt.batch}, '
             f'conf_thres 0.001; {masks["tp"] + masks["fp"]} predicted instances own a pixel; {opt.repeats} repeats per path, alternated, after one warm-up pass each',
             f'box fitness: bank {last["bank"][0]:.6f}, float {last["float"][0]:.6f}',
             'ms per image            median      min      max']
    for k in paths:
        for i, name in enumerate(('pre', 'infer+nms', 'metrics')):
            v = [s[i] for s in speeds[k]]
            lines.append(f'{k:6s} {name:10s} {statistics.median(v):12.3f} {min(v):8.3f} {max(v):8.3f}')
        v = [sum(s) for s in speeds[k]]
        lines.append(f'{k:6s} {"total":10s} {statistics.median(v):12.3f} {min(v):8.3f} {max(v):8.3f}')
    report = '\n'.join(lines) + '\n'
    print(report, end='')
    if opt.out:
        with open(opt.out, 'w') as f:
            f.write(report)


if __name__ == '__main__':
    main()
