"""Train step of yolov5s (nc 8, 64 x 640^2, bf16) under three loss forms, in one process, alternated:
  default      BCE on the fused loss (csrc/loss.hip)
  focal        fl_gamma 1.5 on the fused loss
  focal_eager  fl_gamma 1.5 with HDY_FUSED_LOSS=0: the tensor-expression DetLoss (matcher, CIoU, focal BCE and scatter as torch ops + autograd)
Every case is warmed up first (plans built, code objects loaded); then `--rounds` rounds each time `--steps` steps of every case in turn.
Prints one JSON line: per case the median ms per step over the rounds and the spread (min, max).
Usage: python scripts/bench_loss_forms.py [--steps 10] [--rounds 7] [--warmup 3] [--cases default,focal,focal_eager]"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault('YOLOv5_VERBOSE', 'false')
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from hd_yolo_amd import synth  # noqa: E402
from hd_yolo_amd.optim import SGD  # noqa: E402

CASES = {'default': (0.0, '1'), 'focal': (1.5, '1'), 'focal_eager': (1.5, '0')}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--size', type=int, default=640)
    ap.add_argument('--cases', default=','.join(CASES))
    args = ap.parse_args()
    from metayolo.models.yolo import Model
    dev = torch.device('cuda', 0)
    nc = 8
    x = synth.synth_images(args.batch, args.size, seed=0).to(dev)
    targets = synth.synth_targets(args.batch, args.size, nc, seed=1)
    for t in targets:
        for a in t['anns']['det']:
            a['boxes'], a['labels'] = a['boxes'].to(dev), a['labels'].to(dev)
    models = {}
    for gamma in sorted({CASES[c][0] for c in args.cases.split(',')}):
        hyp = synth.make_hyp()
        hyp['det']['fl_gamma'] = gamma
        m = Model(synth.make_cfg('s', nc), hyp)
        m.load_state_dict(synth.synth_state_dict(synth.shapes_of(m), seed=0), strict=False)
        m = m.to(dev).train().half()
        opt = SGD([p for p in m.parameters()], lr=1e-4, momentum=0.937, nesterov=True)
        models[gamma] = (m, opt)

    def step(case):
        gamma, fused = CASES[case]
        os.environ['HDY_FUSED_LOSS'] = fused
        m, opt = models[gamma]
        losses, _ = m(x, targets, compute_masks=False)
        losses['det']['det_loss'].backward()
        opt.step()
        opt.zero_grad(set_to_none=True)

    cases = args.cases.split(',')
    for c in cases:
        for _ in range(args.warmup):
            step(c)
    torch.cuda.synchronize()
    times = {c: [] for c in cases}
    for _ in range(args.rounds):
        for c in cases:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step(c)
            torch.cuda.synchronize()
            times[c].append((time.perf_counter() - t0) / args.steps * 1e3)
    os.environ.pop('HDY_FUSED_LOSS', None)
    out = {'config': f'yolov5s nc={nc} {args.batch}x{args.size}^2 bf16 train step, {args.rounds} rounds x {args.steps} steps, alternated'}
    for c in cases:
        v = np.array(times[c])
        out[c] = {'median_ms': round(float(np.median(v)), 3), 'min_ms': round(float(v.min()), 3), 'max_ms': round(float(v.max()), 3)}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
