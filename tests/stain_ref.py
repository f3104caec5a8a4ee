"""Numpy restatement of the four passes of include/hdyolo_stain.h, in int64 and straight from the header's definitions, and a float64 "ideal"
Macenko estimate and recolouring to measure the integer method against.  The passes here import nothing of hd_yolo_amd.stain; RefCounts puts
them behind the three calls hd_yolo_amd.stain.estimate_from_counts makes, so that the estimator can run on these counts.

Why a recoloured byte is within 1 of round() of the ideal.  The ideal byte of a channel is x = 256 * 10^-od' - 1 (real, clipped to [0, 255])
with od' = N od.  The pass takes the index i = floor(T od' / od_top + d), |d| <= 1.5 * 2^-16 (three table entries, each rounded by at most
half a unit of 2^-16 of a step), and the byte tone[i] = round(256 * 10^-((i + 0.5) od_top / T)) - 1.  The optical density at the centre of
step i differs from od' by at most (0.5 + 1.5 * 2^-16) od_top / T, and |d/d od (256 * 10^-od)| <= 256 ln 10, so before its rounding the
table's value differs from x by at most 256 ln 10 * 0.50003 * od_top / T = 0.0867 at T = 8192 (a whole step: 0.174 < 0.18 byte); with the
table's own rounding |tone[i] - x| <= 0.587 and |tone[i] - round(x)| <= 1.087, which between integers means at most 1.  Below od' = 0 both
sides clip to 255, above od_top both to 0."""
import math

import numpy as np

OD_SHIFT, ANGLE_SHIFT, SHIFT = 10, 4, 16
MAX_BINS, MAX_TONE = 1024, 8192
OD_TOP = math.log10(256.0)


def od_exact():
    return -np.log10((np.arange(256) + 1) / 256.0)


def od_table():
    return np.rint((1 << OD_SHIFT) * od_exact()).astype(np.int64)


def visited(rgb, window=None, step=1):
    """(ny, nx, 3) uint8: the pixels (x0 + i step, y0 + j step) of the window"""
    H, W = rgb.shape[:2]
    x0, y0, w, h = (0, 0, W, H) if window is None else window
    assert 0 <= x0 and 0 <= y0 and w >= 1 and h >= 1 and x0 + w <= W and y0 + h <= H and step >= 1
    return rgb[y0:y0 + h:step, x0:x0 + w:step, :3]


def tissue_pixels(rgb, window=None, step=1, background=220):
    """(n, 3) int64: the visited pixels with min(R, G, B) < background"""
    px = visited(rgb, window, step).reshape(-1, 3).astype(np.int64)
    return px[px.min(1) < background]


def wrap32(t):
    """an int64 array as 32-bit two's complement"""
    return ((np.asarray(t, np.int64) + (1 << 31)) % (1 << 32)) - (1 << 31)


def table_sum(lut3, px):
    """lut3 (3, 256), px (n, 3) -> (n,) int64: lut[0][R] + lut[1][G] + lut[2][B] modulo 2^32"""
    lut3 = np.asarray(lut3, np.int64)
    return wrap32(lut3[0][px[:, 0]] + lut3[1][px[:, 1]] + lut3[2][px[:, 2]])


def moments(rgb, od, window=None, step=1, background=220):
    q = np.asarray(od, np.int64)[tissue_pixels(rgb, window, step, background)]
    r, g, b = q[:, 0], q[:, 1], q[:, 2]
    return np.array([len(q), r.sum(), g.sum(), b.sum(), (r * r).sum(), (r * g).sum(), (r * b).sum(), (g * g).sum(), (g * b).sum(), (b * b).sum()],
                    np.int64)


def angle_bins(p0, p1, A):
    """the bin of every pixel with p0 > 0 (int64 arrays): floor(A (s + p1) / (2 s)), s = p0 + |p1|"""
    s = p0 + np.abs(p1)
    return (A * (s + p1)) // (2 * s)


def angles(rgb, lut, A, window=None, step=1, background=220):
    px = tissue_pixels(rgb, window, step, background)
    lut = np.asarray(lut, np.int64)
    p0, p1 = table_sum(lut[0], px) >> ANGLE_SHIFT, table_sum(lut[1], px) >> ANGLE_SHIFT
    keep = p0 > 0
    bins = angle_bins(p0[keep], p1[keep], A)
    assert not len(bins) or (0 <= bins.min() and bins.max() < A)
    return np.bincount(bins, minlength=A).astype(np.int64), np.array([(~keep).sum()], np.int64)


def levels(rgb, lut, B, window=None, step=1, background=220):
    px = tissue_pixels(rgb, window, step, background)
    lut = np.asarray(lut, np.int64)
    return np.stack([np.bincount(np.clip(table_sum(lut[s], px) >> SHIFT, 0, B - 1), minlength=B) for s in range(2)]).astype(np.int64)


def apply(rgb, lut, tone, window=None, out=None, out_channels=None):
    """the recoloured image: `out` (a copy is made; None = 0x7F bytes of the slide's H x W and out_channels or the input's channels) with the
    window's pixels written"""
    H, W, C = rgb.shape
    x0, y0, w, h = (0, 0, W, H) if window is None else window
    out = np.full((H, W, out_channels or C), 0x7F, np.uint8) if out is None else out.copy()
    lut, tone = np.asarray(lut, np.int64), np.asarray(tone, np.uint8)
    T = len(tone)
    src = rgb[y0:y0 + h, x0:x0 + w]
    px = src[..., :3].reshape(-1, 3).astype(np.int64)
    new = np.stack([tone[np.clip(table_sum(lut[c], px) >> SHIFT, 0, T - 1)] for c in range(3)], 1).reshape(h, w, 3)
    dst = out[y0:y0 + h, x0:x0 + w]
    dst[..., :3] = new
    if out.shape[2] == 4:
        dst[..., 3] = src[..., 3] if C == 4 else 255
    return out


class RefCounts:
    """the three counting passes above behind the calls of hd_yolo_amd.stain.estimate_from_counts (torch tensors in and out)"""

    def __init__(self, rgb, window=None, step=1, background=220):
        self.rgb, self.args = rgb, (window, step, background)

    def moments(self, od):
        import torch
        return torch.from_numpy(moments(self.rgb, od.numpy(), *self.args))

    def angles(self, lut, A):
        import torch
        return tuple(torch.from_numpy(v) for v in angles(self.rgb, lut.numpy(), A, *self.args))

    def levels(self, lut, B):
        import torch
        return torch.from_numpy(levels(self.rgb, lut.numpy(), B, *self.args))


# ---- the float64 ideal ------------------------------------------------------------------------------------------------------------------------
def rank(a, n):
    return max(1, math.ceil(round(a * n, 9)))


def ideal_estimate(rgb, alpha=0.01, window=None, step=1, background=220):
    """(matrix (3, 3), max_conc (2,)) by Macenko's method in float64 on the exact optical densities: exact angles and exact concentrations,
    the order statistics taken by sorting under the rank rule of the integer method (the value at position rank(a, n) of the sorted list)"""
    od = od_exact()[tissue_pixels(rgb, window, step, background)]
    n = len(od)
    lam, vec = np.linalg.eigh(np.cov(od.T, bias=True))
    e1, e2 = vec[:, 2], vec[:, 1]
    e1 = -e1 if e1 @ od.mean(0) < 0 else e1
    e2 = -e2 if e2[0] < 0 else e2
    p0, p1 = od @ e1, od @ e2
    phi = np.sort(np.arctan2(p1[p0 > 0], p0[p0 > 0]))
    lo, hi = phi[rank(alpha, len(phi)) - 1], phi[rank(1 - alpha, len(phi)) - 1]
    va, vb = (e1 * math.cos(p) + e2 * math.sin(p) for p in (lo, hi))
    h, e = (va, vb) if va[0] >= vb[0] else (vb, va)
    r = np.cross(h, e)
    matrix = np.stack([h / np.linalg.norm(h), e / np.linalg.norm(e), r / np.linalg.norm(r)])
    conc = od @ np.linalg.inv(matrix)
    k = rank(1 - alpha, n) - 1
    return matrix, np.array([np.sort(conc[:, 0])[k], np.sort(conc[:, 1])[k]])


def ideal_recolour(rgb, N):
    """float64 (H, W, 3): 256 * 10^-(N od) - 1 per pixel, clipped to [0, 255] and not rounded"""
    od = od_exact()[rgb[..., :3].astype(np.int64)]
    return np.clip(256 * 10.0 ** -(od @ np.asarray(N, np.float64).T) - 1, 0, 255)


def angle_deg(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return math.degrees(math.acos(max(-1.0, min(1.0, float(a @ b) / float(np.linalg.norm(a) * np.linalg.norm(b))))))
