"""numpy restatements of include/hdyolo_texture.h (hdy_label_texture) and of the features hd_yolo_amd/texture.py derives from its counts.

texture_loop is the header read aloud: a loop over the entries of every label's clamped box.  texture_vec states the same with whole-array
operations (np.add.at), so that two builds of one statement can be held against each other.  haralick_loop and intensity_loop are written
from the definitions (Haralick, Shanmugam, Dinstein 1973; the conventions of the issue that introduced them), entry by entry, in plain
Python floats: nothing of hd_yolo_amd is imported here.
"""
import math

import numpy as np

MAX_SIDE, SHIFT = 1024, 16


def levels_of(rgb, lut, levels):
    """int64 (h, w): the level of every pixel of an (h, w, 3) uint8 window.  The sum of the three entries wraps modulo 2^32."""
    lut = np.asarray(lut, dtype=np.int64)
    t = lut[0][rgb[..., 0]] + lut[1][rgb[..., 1]] + lut[2][rgb[..., 2]]
    t = ((t + (1 << 31)) % (1 << 32)) - (1 << 31)                        # 32-bit two's complement
    return np.clip(t >> SHIFT, 0, levels - 1)                            # >> on int64 is the floor


def clamp_box(extent_row, h, w):
    bx0, by0 = max(int(extent_row[0]), 0), max(int(extent_row[1]), 0)
    bx1, by1 = min(int(extent_row[2]), w - 1), min(int(extent_row[3]), h - 1)
    bw, bh = bx1 - bx0 + 1, by1 - by0 + 1
    flag = 1 if bw < 1 or bh < 1 else 2 if bw > MAX_SIDE or bh > MAX_SIDE else 0
    return bx0, by0, bx1, by1, flag


def texture_loop(label_map, rgb, extent, lut, levels, offsets, row0=0, rows=None):
    """(hist (rows, L), glcm (rows, D, L, L), flags (rows,)) int32: the header, entry by entry.  rgb: the (h, w, 3) window under the map."""
    h, w = label_map.shape
    R = len(extent)
    rows = R - row0 if rows is None else rows
    D = len(offsets)
    lev = levels_of(rgb, lut, levels)
    hist = np.zeros((rows, levels), np.int64)
    glcm = np.zeros((rows, D, levels, levels), np.int64)
    flags = np.zeros((rows,), np.int64)
    for q in range(rows):
        r = row0 + q
        bx0, by0, bx1, by1, flags[q] = clamp_box(extent[r], h, w)
        if flags[q]:
            continue
        for i in range(by0, by1 + 1):
            for j in range(bx0, bx1 + 1):
                if label_map[i, j] != r:
                    continue
                a = lev[i, j]
                hist[q, a] += 1
                for d, (di, dj) in enumerate(offsets):
                    ni, nj = i + di, j + dj
                    if 0 <= ni < h and 0 <= nj < w and label_map[ni, nj] == r:
                        b = lev[ni, nj]
                        glcm[q, d, a, b] += 1
                        glcm[q, d, b, a] += 1
    return hist.astype(np.int32), glcm.astype(np.int32), flags.astype(np.int32)


def texture_vec(label_map, rgb, extent, lut, levels, offsets, row0=0, rows=None):
    """the same statement with whole-array operations: per label a mask of its box, per offset a shifted comparison, np.add.at"""
    h, w = label_map.shape
    R = len(extent)
    rows = R - row0 if rows is None else rows
    D = len(offsets)
    lev = levels_of(rgb, lut, levels)
    hist = np.zeros((rows, levels), np.int64)
    glcm = np.zeros((rows, D, levels, levels), np.int64)
    flags = np.zeros((rows,), np.int64)
    ii, jj = np.mgrid[0:h, 0:w]
    for q in range(rows):
        r = row0 + q
        bx0, by0, bx1, by1, flags[q] = clamp_box(extent[r], h, w)
        if flags[q]:
            continue
        own = label_map == r
        src = own & (ii >= by0) & (ii <= by1) & (jj >= bx0) & (jj <= bx1)
        hist[q] = np.bincount(lev[src], minlength=levels)
        si, sj = np.nonzero(src)
        for d, (di, dj) in enumerate(offsets):
            ni, nj = si + di, sj + dj
            ok = (ni >= 0) & (ni < h) & (nj >= 0) & (nj < w)
            ok[ok] = own[ni[ok], nj[ok]]
            a, b = lev[si[ok], sj[ok]], lev[ni[ok], nj[ok]]
            np.add.at(glcm[q, d], (a, b), 1)
            np.add.at(glcm[q, d], (b, a), 1)
    return hist.astype(np.int32), glcm.astype(np.int32), flags.astype(np.int32)


def _h(values):
    """-sum v log v with 0 log 0 = 0"""
    return -sum(v * math.log(v) for v in values if v > 0)


def haralick_loop(g):
    """the 13 features of one (L, L) matrix of counts as a list of floats, from the definitions; 13 NaN for a matrix without pairs.
    Levels 0 .. L - 1, natural logarithms, variances about the mean; correlation 1 where sx sy = 0; imc1 0 where max(HX, HY) = 0."""
    L = len(g)
    total = sum(int(g[i][j]) for i in range(L) for j in range(L))
    if total == 0:
        return [float('nan')] * 13
    p = [[int(g[i][j]) / total for j in range(L)] for i in range(L)]
    px = [sum(p[i][j] for j in range(L)) for i in range(L)]
    py = [sum(p[i][j] for i in range(L)) for j in range(L)]
    mx = sum(i * px[i] for i in range(L))
    my = sum(j * py[j] for j in range(L))
    sx = math.sqrt(sum((i - mx) ** 2 * px[i] for i in range(L)))
    sy = math.sqrt(sum((j - my) ** 2 * py[j] for j in range(L)))
    psum = [0.0] * (2 * L - 1)
    pdif = [0.0] * L
    for i in range(L):
        for j in range(L):
            psum[i + j] += p[i][j]
            pdif[abs(i - j)] += p[i][j]
    f = [0.0] * 13
    f[0] = sum(p[i][j] ** 2 for i in range(L) for j in range(L))
    f[1] = sum((i - j) ** 2 * p[i][j] for i in range(L) for j in range(L))
    cov = sum((i - mx) * (j - my) * p[i][j] for i in range(L) for j in range(L))
    f[2] = cov / (sx * sy) if sx * sy > 0 else 1.0
    f[3] = sum((i - mx) ** 2 * p[i][j] for i in range(L) for j in range(L))
    f[4] = sum(p[i][j] / (1 + (i - j) ** 2) for i in range(L) for j in range(L))
    f[5] = sum(k * psum[k] for k in range(2 * L - 1))
    f[6] = sum((k - f[5]) ** 2 * psum[k] for k in range(2 * L - 1))
    f[7] = _h(psum)
    f[8] = _h(p[i][j] for i in range(L) for j in range(L))
    dmean = sum(k * pdif[k] for k in range(L))
    f[9] = sum((k - dmean) ** 2 * pdif[k] for k in range(L))
    f[10] = _h(pdif)
    hx, hy = _h(px), _h(py)
    hxy1 = -sum(p[i][j] * math.log(px[i] * py[j]) for i in range(L) for j in range(L) if p[i][j] > 0)
    hxy2 = -sum(px[i] * py[j] * math.log(px[i] * py[j]) for i in range(L) for j in range(L) if px[i] * py[j] > 0)
    f[11] = (f[8] - hxy1) / max(hx, hy) if max(hx, hy) > 0 else 0.0
    f[12] = math.sqrt(max(1 - math.exp(-2 * (hxy2 - f[8])), 0.0))
    return f


def intensity_loop(hist):
    """[mean, std, skewness, kurtosis, entropy, min, median, max] of one histogram of levels; 8 NaN for an empty one.  Population moments;
    skewness = m3 / std^3 and kurtosis = m4 / std^4, both 0 where std = 0; the median is the lowest level at which the cumulative count
    reaches half of the pixels."""
    c = [int(v) for v in hist]
    n = sum(c)
    if n == 0:
        return [float('nan')] * 8
    p = [v / n for v in c]
    mean = sum(k * p[k] for k in range(len(c)))
    m2, m3, m4 = (sum((k - mean) ** e * p[k] for k in range(len(c))) for e in (2, 3, 4))
    std = math.sqrt(m2)
    used = [k for k in range(len(c)) if c[k]]
    run, med = 0, 0
    for k in range(len(c)):
        run += c[k]
        if 2 * run >= n:
            med = k
            break
    return [mean, std, m3 / std ** 3 if std > 0 else 0.0, m4 / std ** 4 if std > 0 else 0.0, _h(p), float(used[0]), float(med), float(used[-1])]
