"""The stain passes on the MI355X (csrc/stain.hip), measured: each of the four passes alone (one call into buffers made beforehand) and the
whole stain.normalize_slide (estimate: three counting passes, eigenvectors and percentiles on the host; then the recolouring) on synthetic
stained slides, alternating with hdy_slide_tissue_u8 over the same slide (the yardstick: one streaming pass over the same bytes, one
workgroup per 256 x 256 tile) and against what a user would write without the passes: the same counts as chunked tensor expressions (table
gathers, masked sums, torch.bincount per chunk of rows).

    python scripts/bench_stain.py [--out profiles/stain_ab.txt] [--repeats 7] [--sides 4096 16384]

The slide is synth.synth_stained_slide(1024, ...) of turned stain vectors, repeated to the side: blobs of haematoxylin on an eosin ground and
40 % white background, so that most pixels fall into a few dozen of the 1024 bins, as on tissue.  Device time between events; the candidates
alternate inside every repeat.  Before anything is timed the kernels' counts are checked equal to the tensor expressions'."""
import argparse
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

from bench_paste import events, stats  # noqa: E402
from hd_yolo_amd import ops, synth  # noqa: E402
from hd_yolo_amd import stain as hstain  # noqa: E402
from hd_yolo_amd import texture as htexture  # noqa: E402

BINS, TILE, CHUNK_PIXELS, BACKGROUND = 1024, 256, 1 << 24, 220


def turned(v, axis, deg):
    v, k, t = np.asarray(v, float), np.asarray(axis, float) / np.linalg.norm(axis), math.radians(deg)
    return v * math.cos(t) + np.cross(k, v) * math.sin(t) + k * (k @ v) * (1 - math.cos(t))


def table_sum(lut3, px):
    return (lut3[0][px[..., 0]] + lut3[1][px[..., 1]] + lut3[2][px[..., 2]]).to(torch.int32)      # modulo 2^32, as the passes


def tensor_counts(slide, od, plane, levels):
    """(sums, angle hist, skipped, level hist) as tensor expressions over chunks of rows"""
    H, W, _ = slide.shape
    dev = slide.device
    sums = torch.zeros(10, dtype=torch.int64, device=dev)
    hist = torch.zeros(BINS, dtype=torch.int64, device=dev)
    skipped = torch.zeros(1, dtype=torch.int64, device=dev)
    lv = torch.zeros((2, BINS), dtype=torch.int64, device=dev)
    rows = max(1, CHUNK_PIXELS // W)
    for r0 in range(0, H, rows):
        px = slide[r0:r0 + rows, :, :3].reshape(-1, 3)
        px = px[px.amin(1) < BACKGROUND].long()
        q = od.long()[px]
        r, g, b = q[:, 0], q[:, 1], q[:, 2]
        sums += torch.stack([torch.tensor(len(q), device=dev), r.sum(), g.sum(), b.sum(), (r * r).sum(), (r * g).sum(), (r * b).sum(), (g * g).sum(),
                             (g * b).sum(), (b * b).sum()])
        p0, p1 = (table_sum(plane[k], px) >> hstain.ANGLE_SHIFT for k in range(2))
        keep = p0 > 0
        p0, p1 = p0[keep].long(), p1[keep].long()
        s = p0 + p1.abs()
        hist += torch.bincount((BINS * (s + p1)) // (2 * s), minlength=BINS)
        skipped += (~keep).sum()
        for k in range(2):
            lv[k] += torch.bincount((table_sum(levels[k], px) >> hstain.SHIFT).clamp_(0, BINS - 1).long(), minlength=BINS)
    return sums, hist, skipped, lv


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='')
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--sides', type=int, nargs='*', default=[4096, 16384])
    opt = ap.parse_args()
    dev = torch.device('cuda', 0)
    med = statistics.median
    m0 = htexture.stain_matrix().numpy()
    vectors = np.stack([turned(m0[0], (0, 0, 1), 7), turned(m0[1], (1, 0, 0), -6)])
    tile = torch.from_numpy(synth.synth_stained_slide(1024, vectors, (0.9, 0.5), seed=1)).to(dev)
    lines = ['command: python ' + ' '.join(sys.argv),
             f'device: {torch.cuda.get_device_name(0)}; ms, median [min .. max] over {opt.repeats} repeats, device time between events, candidates '
             f'alternating inside every repeat; RGB slides, step 1, {BINS} angle bins and {BINS} levels per stain, tone table of 8192; x = time over '
             f'the slide_tissue yardstick (same bytes read, one workgroup per {TILE} x {TILE} tile)',
             f'tensor expressions: the three counts by table gathers, masked sums and torch.bincount per {CHUNK_PIXELS} pixels', '']
    names = ('tissue', 'moments', 'angles', 'levels', 'apply', 'normalize', 'tensor')
    head = {'tissue': 'slide_tissue (yardstick)', 'moments': 'stain_moments', 'angles': 'stain_angles', 'levels': 'stain_levels',
            'apply': 'stain_apply (new slide)', 'normalize': 'normalize_slide (whole)', 'tensor': 'tensor expressions (3 counts)'}
    lines.append(f'{"side":>6s} {"tissue px":>11s}  ' + '  '.join(f'{head[k]:>32s}' + ('' if k in ('tissue', 'tensor') else f' {"x":>6s}') for k in names))
    for side in opt.sides:
        k = (side + 1023) // 1024
        slide = tile.repeat(k, k, 1)[:side, :side].contiguous()
        est = hstain.estimate_stains(slide)
        assert est.flags == 0
        od, levels = hstain.od_table(dev), hstain.level_lut(est.matrix, BINS, 4.0, dev)
        e1 = est.matrix[0] + est.matrix[1]                                   # an orthonormal pair in the estimated stain plane
        e1 = e1 / e1.norm()
        e2 = est.matrix[0] - e1 * float(est.matrix[0] @ e1)
        plane = hstain.plane_lut(e1, e2 / e2.norm(), dev)
        lut, tone = hstain.normalizer(est, device=dev)
        origins = ops.slide_origins([(x, y) for y in range(0, side, TILE) for x in range(0, side, TILE)], dev)
        sums, (hist, skipped), lv = ops.stain_moments(slide, od), ops.stain_angles(slide, plane, BINS), ops.stain_levels(slide, levels, BINS)
        want = tensor_counts(slide, od, plane, levels)
        assert all(torch.equal(a, b) for a, b in zip((sums, hist, skipped, lv), want)), 'the kernels and the tensor expressions count differently'
        assert int(ops.slide_tissue(slide, origins, TILE, TILE, BACKGROUND).sum()) == int(sums[0])
        out = torch.empty_like(slide)
        run = {'tissue': lambda: ops.slide_tissue(slide, origins, TILE, TILE, BACKGROUND),
               'moments': lambda: ops.stain_moments(slide, od, out=sums),
               'angles': lambda: ops.stain_angles(slide, plane, BINS, out=(hist, skipped)),
               'levels': lambda: ops.stain_levels(slide, levels, BINS, out=lv),
               'apply': lambda: ops.stain_apply(slide, lut, tone, out=out),
               'normalize': lambda: hstain.normalize_slide(slide, out=out),
               'tensor': lambda: tensor_counts(slide, od, plane, levels)}
        for fn in run.values():
            fn()
        t = {k: [] for k in names}
        for _ in range(opt.repeats):
            for name in names:
                if name != 'tissue':
                    t['tissue'].append(events(run['tissue'])[0])
                    t[name].append(events(run[name])[0])
        y = med(t['tissue'])
        lines.append(f'{side:6d} {int(sums[0]):11d}  ' + '  '.join(f'{stats(t[k]):>32s}' + ('' if k in ('tissue', 'tensor') else f' {med(t[k]) / y:5.2f}x')
                                                                  for k in names))
        print(lines[-1], flush=True)
        del slide, out
        torch.cuda.empty_cache()
    text = '\n'.join(lines)
    print(text)
    if opt.out:
        with open(opt.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
