"""Texture counts on the MI355X (csrc/texture.hip), measured: hdy_label_texture alone (one launch over all labels into buffers made
beforehand) and the whole texture.texture_table (table, chunked launches, intensity and Haralick columns) on the label map of a synthetic
slide of 10^4 .. 2.5 x 10^5 nuclei at 16 levels and 4 offsets, alternating with hdy_label_measure on the same map and image (the yardstick:
one streaming pass over the same map and pixel bytes), and against what a user would write without the pass: the same histograms and
matrices as chunked tensor expressions (levels by table gather, pair indices from shifted maps, torch.bincount per chunk of labels).

    python scripts/bench_texture.py [--out profiles/texture_ab.txt] [--repeats 7] [--sizes 10000 100000 250000] [--chunk 16384]

Slides at nucleus density (bench_paste.py's: one object per 40 x 40 px), pasted into one int32 label map with elliptic 28 x 28 patches; the
image is smooth at the scale of a nucleus (a random field at a quarter of the resolution plus noise), so that a nucleus uses a few
neighbouring levels, as chromatin does.  Device time between events; the candidates alternate inside every repeat.  Before anything is timed the
kernel's counts are checked equal to the tensor expressions'."""
import argparse
import ctypes
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

from bench_paste import events, slide_case, stats  # noqa: E402
from hd_yolo_amd import _ext, ops  # noqa: E402
from hd_yolo_amd import texture as htexture  # noqa: E402

L, OFFSETS = 16, htexture.OFFSETS


def smooth_image(side, dev, seed):
    g = torch.Generator(dev).manual_seed(seed)
    q = (side + 3) // 4
    coarse = torch.randint(0, 256, (q, q, 3), device=dev, generator=g, dtype=torch.int16)
    fine = coarse.repeat_interleave(4, 0).repeat_interleave(4, 1)[:side, :side]
    noise = torch.randint(-12, 13, (side, side, 3), device=dev, generator=g, dtype=torch.int16)
    return (fine + noise).clamp_(0, 255).to(torch.uint8).contiguous()


def tensor_texture(lm, R, image, lut, chunk):
    """(hist, glcm) as tensor expressions: the level of every pixel by table gather, per offset the entries whose partner holds the same
    label, one bincount per chunk of labels (so that at most chunk * D * L * L bins exist at once), the matrix plus its transpose"""
    h, w = lm.shape
    px = image[..., :3].long()
    lev = ((lut[0][px[..., 0]] + lut[1][px[..., 1]] + lut[2][px[..., 2]]) >> htexture.SHIFT).clamp_(0, L - 1).long()
    own = (lm >= 0) & (lm < R)
    lab = lm.long()
    D = len(OFFSETS)
    hidx = (lab * L + lev)[own]
    pidx = []
    for d, (di, dj) in enumerate(OFFSETS):
        ys, yd = (slice(max(-di, 0), h - max(di, 0)), slice(max(di, 0), h - max(-di, 0)))
        xs, xd = (slice(max(-dj, 0), w - max(dj, 0)), slice(max(dj, 0), w - max(-dj, 0)))
        pair = own[ys, xs] & (lm[ys, xs] == lm[yd, xd])
        pidx.append((((lab[ys, xs] * D + d) * L + lev[ys, xs]) * L + lev[yd, xd])[pair])
    pidx = torch.cat(pidx)
    hist = torch.bincount(hidx, minlength=R * L).view(R, L).to(torch.int32)
    glcm = torch.empty((R, D, L, L), dtype=torch.int32, device=lm.device)
    per = D * L * L
    for lo in range(0, R, chunk):
        n = min(chunk, R - lo)
        sel = pidx[(pidx >= lo * per) & (pidx < (lo + n) * per)] - lo * per
        g = torch.bincount(sel, minlength=n * per).view(n, D, L, L)
        glcm[lo:lo + n] = (g + g.transpose(2, 3)).to(torch.int32)
    return hist, glcm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='')
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--sizes', type=int, nargs='*', default=[10000, 100000, 250000])
    ap.add_argument('--chunk', type=int, default=16384)
    opt = ap.parse_args()
    dev = torch.device('cuda', 0)
    med = statistics.median
    D = len(OFFSETS)
    lines = ['command: python ' + ' '.join(sys.argv),
             f'device: {torch.cuda.get_device_name(0)}; ms, median [min .. max] over {opt.repeats} repeats, device time between events, candidates '
             f'alternating inside every repeat; {L} levels, {D} offsets, haematoxylin table; x = time over the label_measure yardstick',
             f'tensor expressions: table gather, shifted-map pair indices, torch.bincount per {opt.chunk} labels (counts only, no features)', '']
    lines.append(f'{"labels":>8s} {"canvas":>7s} {"owned":>10s} {"pairs":>10s}  {"label_measure, RGB (yardstick)":>34s}  {"label_texture launch":>34s} {"x":>6s}  '
                 f'{"texture_table (counts + columns)":>34s}  {"tensor expressions (counts)":>34s}  {"kernel speed-up":>15s}')
    for n in opt.sizes:
        boxes, masks, side = slide_case(n, dev)
        R = len(boxes)
        lm = ops.paste_label_map(masks, boxes, (side, side))
        del masks
        image = smooth_image(side, dev, n)
        lut = htexture.stain_lut('hematoxylin', L, device=dev)
        sums, extent = ops.label_measure(lm, R, image=image)
        hist, glcm, flags = ops.label_texture(lm, R, extent, image, lut, L, OFFSETS)
        h_t, g_t = tensor_texture(lm, R, image, lut, opt.chunk)
        assert torch.equal(hist, h_t) and torch.equal(glcm, g_t), 'the kernel and the tensor expressions count differently'
        assert not bool((flags == 2).any()) and torch.equal(hist.sum(1).long(), sums[:, 0])
        pairs = int(glcm.sum(dtype=torch.int64)) // 2
        del h_t, g_t
        host = (ctypes.c_int * (2 * D))(*(v for o in OFFSETS for v in o))
        stream = ops.stream_ptr()

        def launch():
            _ext.call('hdy_label_texture', lm.data_ptr(), lm.numel(), side, side, image.data_ptr(), image.numel(), side * 3, 3, 0, 0, extent.data_ptr(),
                      extent.numel(), R, lut.data_ptr(), 768, L, host, 2 * D, D, 0, R, hist.data_ptr(), hist.numel(), glcm.data_ptr(), glcm.numel(),
                      flags.data_ptr(), flags.numel(), stream)

        table = lambda: htexture.texture_table(lm, R, extent, image, levels=L, offsets=OFFSETS, chunk=opt.chunk)      # noqa: E731
        launch()
        table()
        t = {k: [] for k in ('measure', 'launch', 'table', 'tensor')}
        for _ in range(opt.repeats):
            t['measure'].append(events(lambda: ops.label_measure(lm, R, image=image))[0])
            t['launch'].append(events(launch)[0])
            t['measure'].append(events(lambda: ops.label_measure(lm, R, image=image))[0])
            t['table'].append(events(table)[0])
            t['tensor'].append(events(lambda: tensor_texture(lm, R, image, lut, opt.chunk))[0])
        y = med(t['measure'])
        lines.append(f'{R:8d} {side:7d} {int(sums[:, 0].sum()):10d} {pairs:10d}  {stats(t["measure"]):>34s}  {stats(t["launch"]):>34s} {med(t["launch"]) / y:5.2f}x  '
                     f'{stats(t["table"]):>34s}  {stats(t["tensor"]):>34s}  {med(t["tensor"]) / med(t["launch"]):14.1f}x')
        print(lines[-1], flush=True)
        del lm, image, hist, glcm
        torch.cuda.empty_cache()
    text = '\n'.join(lines)
    print(text)
    if opt.out:
        with open(opt.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
