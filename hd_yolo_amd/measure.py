"""The nucleus table: per-label measurements from the integer sums of ops.label_measure (hdy_label_measure, include/hdyolo_measure.h).

nucleus_table is tensor arithmetic on (R, 14) int64 sums and (R, 4) int32 extents: torch int64 / float64 operations on whole columns, no loop
over rows and no read of a value, on whatever device the sums live (the GPU in the slide path, the CPU in the tests).  With n, Sx, Sy, Sxx, Syy,
Sxy the columns 0-5 (dx = j - ox, dy = i - oy about the label's origin (ox, oy)), E and Eb the columns 6 and 7, Sc and Scc the stain sums:

    area                 n
    centroid_x, _y       ox + Sx / n + offset_x,  oy + Sy / n + offset_y
    bbox                 extent + (offset_x, offset_y, offset_x, offset_y): min x, min y, max x, max y, both inclusive
    central moments      A = n Sxx - Sx^2,  B = n Syy - Sy^2,  C = n Sxy - Sx Sy  (exact integers);  mu20 = A / n^2, mu02 = B / n^2, mu11 = C / n^2
    lambda+-             (mu20 + mu02) / 2 +- sqrt(((mu20 - mu02) / 2)^2 + mu11^2)
    major_axis           4 sqrt(lambda+)                   (the axes of the ellipse with the same second moments)
    minor_axis           4 sqrt(max(lambda-, 0))
    eccentricity         sqrt(1 - lambda- / lambda+), 0 where lambda+ = 0
    orientation          atan2(2 mu11, mu20 - mu02) / 2    (radians, of the major axis against the x axis, y pointing down)
    equivalent_diameter  sqrt(4 n / pi)
    perimeter_edges      E: pixel edges between the label and anything else;  border_edges Eb: those on the window border
    touches_border       Eb > 0
    compactness          16 n / E^2                        (1 for a square, pi / 4 for a large disc)
    mean_rgb             Sc / n
    std_rgb              sqrt(max(n Scc - Sc^2, 0)) / n    (population standard deviation)

A, B, C and n Scc - Sc^2 are formed in int64 and are exact while n <= 2^20 and |dx|, |dy| <= 2^10 (n Sxx <= 2^20 * 2^20 * 2^20 = 2^60): that is
what `origin` is for.  About the window's corner a nucleus at column 20 000 would need 2^20 * n * 4e8 and overflow; about the truncated corner
of its own box the offsets are the size of the nucleus.  Everything after the three exact integers is float64.  A label that owns nothing
(n = 0) has NaN in every ratio column and keeps its empty extent {w, h, -1, -1}.
"""
import math
import os

import torch

from . import _ext

COLS = _ext.CONSTANTS['HDY_MEASURE_COLS']


def nucleus_table(sums, extent, origin=None, offset=(0, 0), labels=None, scores=None, stain=True):
    """dict of per-label columns (see the module docstring) from ops.label_measure's (sums, extent).  origin: the int32 (R, 2) tensor the sums
    were taken about (None = zeros); offset = (x, y) of the measured window in the coordinates the table should speak (the slide's); labels /
    scores: carried along as 'labels' / 'scores'.  stain=False leaves 'mean_rgb' / 'std_rgb' out (a map measured without its image)."""
    if sums.dtype != torch.int64 or sums.dim() != 2 or sums.shape[1] != COLS:
        raise ValueError(f'nucleus_table: sums must be int64 (R, {COLS}), got {sums.dtype} {tuple(sums.shape)}')
    R = sums.shape[0]
    if extent.dtype != torch.int32 or tuple(extent.shape) != (R, 4):
        raise ValueError(f'nucleus_table: extent must be int32 ({R}, 4), got {extent.dtype} {tuple(extent.shape)}')
    f64 = torch.float64
    n, sx, sy, sxx, syy, sxy, edges, border = (sums[:, c] for c in range(8))
    nf = n.to(f64)
    off = torch.tensor([int(offset[0]), int(offset[1])], dtype=torch.int64, device=sums.device)
    org = torch.zeros((R, 2), dtype=torch.int64, device=sums.device) if origin is None else origin.to(device=sums.device, dtype=torch.int64)
    table = {'area': n}
    table['centroid_x'] = org[:, 0].to(f64) + sx.to(f64) / nf + float(int(offset[0]))
    table['centroid_y'] = org[:, 1].to(f64) + sy.to(f64) / nf + float(int(offset[1]))
    ext = extent.to(torch.int64)
    table['bbox'] = torch.where((n > 0)[:, None], ext + torch.cat([off, off])[None, :], ext)
    n2 = nf * nf
    mu20, mu02, mu11 = (n * sxx - sx * sx).to(f64) / n2, (n * syy - sy * sy).to(f64) / n2, (n * sxy - sx * sy).to(f64) / n2
    half, diff = (mu20 + mu02) / 2, (mu20 - mu02) / 2
    root = torch.sqrt(diff * diff + mu11 * mu11)
    lp, lm = half + root, half - root
    table['major_axis'] = 4 * torch.sqrt(lp)
    table['minor_axis'] = 4 * torch.sqrt(torch.clamp(lm, min=0))
    table['eccentricity'] = torch.where(lp == 0, torch.zeros_like(lp), torch.sqrt(1 - lm / lp))
    table['orientation'] = torch.atan2(2 * mu11, mu20 - mu02) / 2
    table['equivalent_diameter'] = torch.sqrt(4 * nf / math.pi)
    table['perimeter_edges'], table['border_edges'], table['touches_border'] = edges, border, border > 0
    ef = edges.to(f64)
    table['compactness'] = 16 * nf / (ef * ef)
    if stain:
        sc, scc = sums[:, 8:11], sums[:, 11:14]
        table['mean_rgb'] = sc.to(f64) / nf[:, None]
        table['std_rgb'] = torch.sqrt(torch.clamp(n[:, None] * scc - sc * sc, min=0).to(f64)) / nf[:, None]
    if labels is not None:
        table['labels'] = labels
    if scores is not None:
        table['scores'] = scores
    return table


def save_nucleus_table(path, table):
    """Write a nucleus table as .npz (one array per column) or .csv (one line per nucleus; bbox and the rgb columns spread over named columns) by
    the extension of `path`.  The table crosses to the host here, in one copy: its columns are joined into one float64 matrix on the device."""
    import numpy as np
    ext = os.path.splitext(path)[1].lower()
    if ext not in ('.npz', '.csv'):
        raise ValueError(f'save_nucleus_table: {path!r} is neither .npz nor .csv')
    names, widths, cols = [], [], []
    for k, v in table.items():
        v = v.reshape(v.shape[0], -1)
        names.append(k)
        widths.append(v.shape[1])
        cols.append(v.to(torch.float64))
    # float64 holds every column exactly: int64 counts and sums of squares stay far below 2^53, labels and booleans are small integers
    R = cols[0].shape[0] if cols else 0
    host = torch.cat(cols, dim=1).cpu().numpy() if cols else np.zeros((0, 0))
    split, at = {}, 0
    for k, wd in zip(names, widths):
        a = host[:, at:at + wd]
        at += wd
        dt = table[k].dtype
        a = a.astype(bool if dt == torch.bool else np.int64 if not dt.is_floating_point else np.float64 if dt == torch.float64 else np.float32)
        split[k] = a.reshape(tuple(table[k].shape))
    if ext == '.npz':
        np.savez(path, **split)
        return
    sub = {'bbox': ('x0', 'y0', 'x1', 'y1'), 'mean_rgb': ('r', 'g', 'b'), 'std_rgb': ('r', 'g', 'b')}
    header, fields = [], []
    for k, wd in zip(names, widths):
        a = split[k].reshape(R, wd)
        for c in range(wd):
            header.append(k if wd == 1 else f'{k}_{sub[k][c] if k in sub else c}')
            fields.append(a[:, c])
    with open(path, 'w') as f:
        f.write(','.join(header) + '\n')
        for i in range(R):
            f.write(','.join(repr(float(v[i])) if v.dtype.kind == 'f' else str(int(v[i])) for v in fields) + '\n')


def load_nucleus_table(path):
    """What save_nucleus_table wrote, as a dict of numpy arrays (.csv: one 1-D array per named column, integers where every value is one)."""
    import numpy as np
    if os.path.splitext(path)[1].lower() == '.npz':
        with np.load(path) as z:
            return {k: z[k] for k in z.files}
    with open(path) as f:
        header = f.readline().strip().split(',')
        rows = [line.strip().split(',') for line in f if line.strip()]
    out = {}
    for c, k in enumerate(header):
        col = [r[c] for r in rows]
        out[k] = np.array([float(v) for v in col], dtype=np.float64) if any(ch in v for v in col for ch in '.enai') else np.array([int(v) for v in col], dtype=np.int64)
    return out
