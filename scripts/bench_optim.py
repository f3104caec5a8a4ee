"""Optimizer step + weight EMA on yolov5s' real parameter set: the one-launch path (hd_yolo_amd.optim `step(ema=ema)`, csrc/optim.hip hdy_opt_step)
against the path it replaces, alternated (reference: train.py:478-480 `optimizer.step(); ema.update(model)` with train.py:228-233's optimizers).

  parent  SGD: hd_yolo_amd.optim.SGD.step() + ModelEMA.update (two calls, the step's launch without the EMA);  Adam / AdamW: torch.optim's step + ModelEMA.update
  fused   hd_yolo_amd.optim.{SGD, Adam, AdamW}.step(ema=ema)

Gradients are views of one flat buffer, as the engine hands them out (engine.GradStore).  Per optimizer and alternation: time per step between
two HIP events around --steps back-to-back steps (whichever of host and device is slower sets it), host time per call (median; the call
returns before the GPU is done), device launches in one step and the time they take on the device (torch profiler), and the bytes the
fused kernel must move — 28 B (SGD + EMA) or 36 B (Adam + EMA) per trained parameter, 12 B per EMA-only entry — over the fused time and
over the fused launch's device time.  The last line per optimizer says whether the fused path beat the parent in every alternation by more
than the parent's own spread across alternations (the rule for making it train.py's default).

    python scripts/bench_optim.py --out profiles/optim_ab.txt
"""
import argparse
import os
import statistics
import sys
import time

os.environ.setdefault('YOLOv5_VERBOSE', 'false')
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from hd_yolo_amd import optim as fused, synth  # noqa: E402
from hd_yolo_amd.engine import GradStore  # noqa: E402
from metayolo.common import ModelEMA  # noqa: E402
from metayolo.models.yolo import Model  # noqa: E402

KW = {'SGD': dict(momentum=0.937, nesterov=True), 'Adam': dict(betas=(0.937, 0.999)), 'AdamW': dict(betas=(0.937, 0.999))}


def setup(name, cls, args, dev):
    """model, train.py's three parameter groups (train.py:213-226), gradients in one flat buffer, EMA"""
    model = Model(synth.make_cfg(args.variant, args.nc), synth.make_hyp()).to(dev).train()
    g_bn, g_w, g_b = [], [], []
    for m in model.modules():
        if hasattr(m, 'bias') and isinstance(m.bias, torch.nn.Parameter):
            g_b.append(m.bias)
        if isinstance(m, torch.nn.BatchNorm2d):
            g_bn.append(m.weight)
        elif hasattr(m, 'weight') and isinstance(m.weight, torch.nn.Parameter):
            g_w.append(m.weight)
    opt = cls(g_bn, lr=1e-4, **KW[name])
    opt.add_param_group({'params': g_w, 'weight_decay': 5e-4})
    opt.add_param_group({'params': g_b})
    store = GradStore(list(model.parameters()), dev)
    store.cur.normal_(generator=torch.Generator(device=dev).manual_seed(0)).mul_(1e-3)
    for p in model.parameters():
        p.grad = store.view_of(p)
    return model, opt, ModelEMA(model), store


def measure(step, steps, dev):
    for _ in range(5):
        step()
    torch.cuda.synchronize(dev)
    host, e0, e1 = [], torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        t = time.perf_counter()
        step()
        host.append(time.perf_counter() - t)
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1) * 1e3 / steps, statistics.median(host) * 1e6


def launches(step, dev):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize(dev)
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize(dev)
    dev_events = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return len(dev_events), sum(e.device_time_total for e in dev_events)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--variant', default='s')
    ap.add_argument('--nc', type=int, default=8)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--alternations', type=int, default=3)
    ap.add_argument('--no-launch-count', action='store_true')
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    assert args.alternations >= 3
    dev = torch.device('cuda', 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f'# {torch.cuda.get_device_name(dev)}, torch {torch.__version__}, yolov5{args.variant} nc={args.nc}, {args.steps} steps per measurement, '
        f'{args.alternations} alternations parent / fused')
    for name in ('SGD', 'Adam', 'AdamW'):
        pm, po, pe, _ps = setup(name, fused.SGD if name == 'SGD' else getattr(torch.optim, name), args, dev)
        fm, fo, fe, _fs = setup(name, getattr(fused, name), args, dev)

        def parent():
            po.step()
            pe.update(pm)

        def one():
            fo.step(ema=fe)
        trained = sum(p.numel() for p in fm.parameters() if p.requires_grad)
        entries = sum(v.numel() for v in fe.ema.state_dict().values() if v.dtype.is_floating_point)
        tensors = sum(1 for v in fe.ema.state_dict().values() if v.dtype.is_floating_point)
        nbytes = (28 if name == 'SGD' else 36) * trained + 12 * (entries - trained)
        say(f'## {name}: {trained} trained parameters in {len(list(fm.parameters()))} tensors, {entries} EMA entries in {tensors} tensors, {nbytes / 1e6:.1f} MB per fused step')
        tp, tf = [], []
        for a in range(args.alternations):
            (gp, hp), (gf, hf) = measure(parent, args.steps, dev), measure(one, args.steps, dev)
            tp.append(gp), tf.append(gf)
            say(f'{name} alternation {a}: parent {gp:8.1f} us/step (host {hp:7.1f} us/call)   fused {gf:8.1f} us/step (host {hf:7.1f} us/call, '
                f'{nbytes / gf / 1e6:6.3f} TB/s)')
        if not args.no_launch_count:
            (np_, dp), (nf, df) = launches(parent, dev), launches(one, dev)
            say(f'{name} device launches in one step (torch profiler): parent {np_} taking {dp:.1f} us on the device, fused {nf} taking {df:.1f} us '
                f'({nbytes / max(df, 1e-9) / 1e6:.3f} TB/s)')
        spread = max(tp) - min(tp)
        wins = all(p - f > spread for p, f in zip(tp, tf))
        say(f'{name}: parent spread {spread:.1f} us, smallest gain {min(p - f for p, f in zip(tp, tf)):.1f} us -> '
            f'{"fused beats parent in every alternation by more than the spread" if wins else "NOT beyond the spread in every alternation"}')
        del pm, po, pe, fm, fo, fe, _ps, _fs
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
