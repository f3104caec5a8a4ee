"""Stain normalisation of an 8-bit slide (Macenko et al. 2009) on the counts of the four passes of include/hdyolo_stain.h.

The passes count and recolour in integers (ops.stain_moments, stain_angles, stain_levels, stain_apply); this module makes their tables and
turns the counts into an estimate, in float64 on the host, from a few hundred bytes read back per slide.

Quantities.  The optical density of a channel value v is od(v) = -log10((v + 1) / 256), as in texture.py; q(v) = round(2^10 od(v)) is its
integer form (od_table).  The rows of a stain matrix M are the unit optical-density vectors of haematoxylin, eosin and their unit cross
product, a pixel's optical density is c M with c its three concentrations, and c = od W with W = inverse(M) (texture.stain_weights).

estimate_stains, step by step:
  1. the covariance of (qR, qG, qB) over the tissue pixels from the ten integer sums, formed exactly: (n S_cd - S_c S_d) / n^2
  2. e1, e2: its two leading eigenvectors (torch.linalg.eigh), e1 negated when e1 . mean < 0, e2 when its R component is negative
  3. the histogram over `bins` of the angle of every tissue pixel in the (e1, e2) plane (plane_lut; the pass's bin is
     floor(bins (s + p_1) / (2 s)), s = p_0 + |p_1|, so the bin centre t = (bin + 0.5) / bins gives u = 2 t - 1 = p_1 / s and the angle
     phi = atan2(u, 1 - |u|)); pixels with p_0 <= 0 are skipped and counted
  4. the lower and upper bin: the lowest bins whose cumulative count reaches rank(alpha, n) and rank(1 - alpha, n), n the histogram's sum,
     rank(a, n) = max(1, ceil(a n)) (the product rounded to 9 decimals first, so that 0.07 * 100 is 7)
  5. the two stain vectors e1 cos phi + e2 sin phi; the one with the larger R component is haematoxylin; the third row is their unit cross
     product
  6. per stain the histogram of the concentration in `bins` levels up to c_top (level_lut); max_conc_s is the centre of the lowest level
     whose cumulative count reaches rank(1 - alpha, n_tissue), in units of c_top / bins
flags (exclusive, the first that applies): 1 fewer than two tissue pixels, 2 a covariance of rank below 2 (or no pixel with p_0 > 0), 3 the
level table is refused because the vectors are nearly parallel.  A flagged estimate carries the target's matrix and max_conc, so that
normalising with it is the identity map up to quantisation.

normalizer.  The recoloured optical density is od' = N od with N = Mt^T diag(r_H, r_E, 0) W^T, that is N[c][d] = sum_s Mt[s][c] r_s
W[d][s], r_s = target.max_conc_s / estimate.max_conc_s; the residual is dropped, as Macenko does.  The pass reads channel c's tone index
floor(T od'_c / od_top) from three table entries (apply_lut) and the byte from tone_table: tone[i] is the byte of the optical density at
the centre of step i, so the byte is within 256 ln 10 od_top / (2 T) + 0.5 < 0.6 of the real-valued 256 * 10^-od' - 1 wherever the three
roundings of the index (1.5 * 2^-16 of a step) do not move it across a step.
"""
import math
from collections import namedtuple

import torch

from . import _ext, texture

OD_SHIFT = _ext.PIXEL_CONSTANTS['HDY_STAIN_OD_SHIFT']
ANGLE_SHIFT = _ext.PIXEL_CONSTANTS['HDY_STAIN_ANGLE_SHIFT']
SHIFT = _ext.PIXEL_CONSTANTS['HDY_STAIN_SHIFT']
MAX_BINS, MAX_TONE = _ext.PIXEL_CONSTANTS['HDY_STAIN_MAX_BINS'], _ext.PIXEL_CONSTANTS['HDY_STAIN_MAX_TONE']
OD_TOP = math.log10(256.0)                                    # od(0): the darkest byte
ENTRY_BOUND = texture.ENTRY_BOUND                             # of level_lut, as stain_lut's
SUM_BOUND = 1 << 31                                           # of apply_lut: the largest magnitudes of a channel's three rows stay below it
FLAG_FEW, FLAG_RANK, FLAG_PARALLEL = 1, 2, 3
RANK_EPS = 1e-12                                              # the second eigenvalue against the first

StainEstimate = namedtuple('StainEstimate', 'matrix max_conc n_tissue n_skipped flags')


class StainTarget(namedtuple('StainTarget', 'matrix max_conc')):
    """The stain model a slide is normalised to.  Default: the Ruifrok-Johnston matrix of texture.stain_matrix() and max_conc = (0.8558,
    0.4477), Macenko's published reference maxima (1.9705, 1.0308) divided by ln 10 (his optical density is a natural logarithm).  A choice,
    not a measurement: any slide of the training set's lab would serve as well."""
    __slots__ = ()

    def __new__(cls, matrix=None, max_conc=(0.8558, 0.4477)):
        m = texture.stain_matrix() if matrix is None else torch.as_tensor(matrix, dtype=torch.float64).cpu()
        return super().__new__(cls, m, torch.as_tensor(max_conc, dtype=torch.float64).cpu())


def _od():
    return -torch.log10((torch.arange(256, dtype=torch.float64) + 1) / 256)


def od_table(device=None):
    """int32 (256,): q(v) = round(2^10 * -log10((v + 1) / 256)); q(255) = 0, q(0) = 2466"""
    return torch.round((1 << OD_SHIFT) * _od()).to(torch.int32).to(device=device)


def plane_lut(e1, e2, device=None):
    """int32 (2, 3, 256) of ops.stain_angles: entry [k][c][v] = round(2^10 e_k[c] q(v)), so that p_k is the projection of (qR, qG, qB) on e_k
    in units of 2^-(10 + 10 - 4) of optical density.  With |e_k[c]| <= 1 no entry passes 2^10 * 2466."""
    e = torch.stack([torch.as_tensor(e1, dtype=torch.float64), torch.as_tensor(e2, dtype=torch.float64)]).cpu()
    if tuple(e.shape) != (2, 3) or not bool((e.abs() <= 1).all()):
        raise ValueError(f'plane_lut: two vectors of three components within [-1, 1] are expected, got {e.tolist()}')
    q = od_table().to(torch.float64)
    return torch.round((1 << 10) * e[:, :, None] * q[None, None, :]).to(torch.int32).to(device=device)


def level_lut(matrix, B, c_top, device=None):
    """int32 (2, 3, 256) of ops.stain_levels: row s is texture.stain_lut's table of stain s (haematoxylin, eosin) of `matrix` at B levels up to
    the concentration c_top.  Refused (ValueError) when an entry reaches 2^28: the sum of three must not wrap."""
    B = int(B)
    if not 1 <= B <= MAX_BINS:
        raise ValueError(f'level_lut: B={B} outside [1, {MAX_BINS}]')
    rows = []
    for stain in ('hematoxylin', 'eosin'):
        coef, value, top = texture.stain_weights(stain, c_top, matrix)
        rows.append(torch.round((1 << SHIFT) * B * coef[:, None] * value[None, :] / top))
    lut = torch.stack(rows)
    if not bool(torch.isfinite(lut).all()) or float(lut.abs().max()) >= ENTRY_BOUND:
        raise ValueError(f'level_lut: an entry reaches 2^28 (B={B}, c_top={c_top}): the stain vectors are nearly parallel')
    return lut.to(torch.int32).to(device=device)


def apply_lut(N, T, device=None):
    """int32 (3, 3, 256) of ops.stain_apply: entry [c][d][v] = round(2^16 T N[c][d] od(v) / od_top), so that channel c's index is
    floor(T od'_c / od_top) with od' = N od.  Refused (ValueError) when the largest magnitudes of a channel's three rows sum to 2^31."""
    T = int(T)
    if not 1 <= T <= MAX_TONE:
        raise ValueError(f'apply_lut: T={T} outside [1, {MAX_TONE}]')
    N = torch.as_tensor(N, dtype=torch.float64).cpu()
    if tuple(N.shape) != (3, 3):
        raise ValueError(f'apply_lut: N must be 3 x 3, got {tuple(N.shape)}')
    lut = torch.round((1 << SHIFT) * T * N[:, :, None] * _od()[None, None, :] / OD_TOP)
    if not bool(torch.isfinite(lut).all()) or float(lut.abs().amax(2).sum(1).max()) >= SUM_BOUND:
        raise ValueError(f'apply_lut: three entries can sum to 2^31 (T={T}): lower T or the concentration ratio')
    return lut.to(torch.int32).to(device=device)


def tone_table(T, device=None):
    """uint8 (T,): tone[i] = clamp(round(256 * 10^(-(i + 0.5) od_top / T)) - 1, 0, 255), the byte at the centre of step i of the optical
    density; non-increasing from 255 to 0"""
    T = int(T)
    if not 1 <= T <= MAX_TONE:
        raise ValueError(f'tone_table: T={T} outside [1, {MAX_TONE}]')
    i = torch.arange(T, dtype=torch.float64)
    return (torch.round(256 * 10 ** (-(i + 0.5) * OD_TOP / T)) - 1).clamp(0, 255).to(torch.uint8).to(device=device)


def rank(a, n):
    """the count the cumulative histogram has to reach for the fraction a of n: max(1, ceil(a n))"""
    return max(1, math.ceil(round(a * n, 9)))


def percentile_bin(hist, k):
    """the lowest bin of the 1-D histogram whose cumulative count reaches k (the last bin when none does)"""
    below = int((torch.cumsum(hist.to(torch.int64), 0) < k).sum())
    return min(below, hist.numel() - 1)


def bin_angle(b, bins):
    """the angle atan2(p_1, p_0) at the centre of bin b of ops.stain_angles"""
    u = 2 * (b + 0.5) / bins - 1
    return math.atan2(u, 1 - abs(u))


class SlideCounts:
    """the three counting passes over one slide on the device (what estimate_from_counts asks of its `counts`)"""

    def __init__(self, slide, window=None, step=1, background=220):
        self.slide, self.args = slide, dict(window=window, step=step, background=background)

    def moments(self, od):
        from . import ops
        return ops.stain_moments(self.slide, od.to(self.slide.device), **self.args)

    def angles(self, lut, A):
        from . import ops
        return ops.stain_angles(self.slide, lut.to(self.slide.device), A, **self.args)

    def levels(self, lut, B):
        from . import ops
        return ops.stain_levels(self.slide, lut.to(self.slide.device), B, **self.args)


def estimate_from_counts(counts, alpha=0.01, bins=1024, c_top=4.0, target=None):
    """StainEstimate from an object with moments(od), angles(lut, A) -> (hist, skipped) and levels(lut, B) (SlideCounts on the device; the
    tests put their numpy restatement of the passes behind the same three calls).  Module docstring for the steps."""
    target = StainTarget() if target is None else target
    bins = int(bins)
    if not 0 < alpha < 0.5 or not 1 <= bins <= MAX_BINS or not c_top > 0:
        raise ValueError(f'estimate_stains: alpha={alpha} (0 .. 0.5), bins={bins} (1 .. {MAX_BINS}), c_top={c_top} (positive)')
    flagged = lambda n, skipped, flag: StainEstimate(target.matrix.clone(), target.max_conc.clone(), n, skipped, flag)      # noqa: E731
    s = [int(v) for v in counts.moments(od_table()).tolist()]
    n = s[0]
    if n < 2:
        return flagged(n, 0, FLAG_FEW)
    first, second = s[1:4], {(0, 0): s[4], (0, 1): s[5], (0, 2): s[6], (1, 1): s[7], (1, 2): s[8], (2, 2): s[9]}
    cov = torch.tensor([[(n * second[min(c, d), max(c, d)] - first[c] * first[d]) / (n * n) for d in range(3)] for c in range(3)],
                       dtype=torch.float64)
    mean = torch.tensor([v / n for v in first], dtype=torch.float64)
    lam, vec = torch.linalg.eigh(cov)                         # ascending
    if not float(lam[2]) > 0 or float(lam[1]) <= RANK_EPS * float(lam[2]):
        return flagged(n, 0, FLAG_RANK)
    e1, e2 = vec[:, 2].clone(), vec[:, 1].clone()
    if float(e1 @ mean) < 0:
        e1 = -e1
    if float(e2[0]) < 0:
        e2 = -e2
    hist, skipped = counts.angles(plane_lut(e1, e2), bins)
    skipped = int(skipped.sum())
    m = int(hist.sum())
    if m < 1:
        return flagged(n, skipped, FLAG_RANK)
    phis = [bin_angle(percentile_bin(hist, rank(a, m)), bins) for a in (alpha, 1 - alpha)]
    va, vb = (e1 * math.cos(p) + e2 * math.sin(p) for p in phis)
    h, e = (va, vb) if float(va[0]) >= float(vb[0]) else (vb, va)
    h, e = h / h.norm(), e / e.norm()
    r = torch.linalg.cross(h, e)
    if not float(r.norm()) > 0:
        return flagged(n, skipped, FLAG_PARALLEL)
    matrix = torch.stack([h, e, r / r.norm()])
    try:
        lut = level_lut(matrix, bins, c_top)
    except (ValueError, RuntimeError):                        # an entry reaches 2^28, or the matrix is singular
        return flagged(n, skipped, FLAG_PARALLEL)
    lv = counts.levels(lut, bins)
    k = rank(1 - alpha, n)
    conc = torch.tensor([(percentile_bin(lv[i], k) + 0.5) * c_top / bins for i in range(2)], dtype=torch.float64)
    return StainEstimate(matrix, conc, n, skipped, 0)


def estimate_stains(slide, window=None, step=1, background=220, alpha=0.01, bins=1024, c_top=4.0, target=None):
    """StainEstimate(matrix float64 (3, 3), max_conc float64 (2,), n_tissue, n_skipped, flags) of an 8-bit slide on the device: Macenko's
    method on the integer counts of three passes over the window's every `step`-th pixel (module docstring).  `target` only supplies what a
    flagged estimate carries."""
    return estimate_from_counts(SlideCounts(slide, window, step, background), alpha, bins, c_top, target)


def transfer_matrix(estimate, target=None):
    """float64 (3, 3) N with od' = N od: N[c][d] = sum_s Mt[s][c] r_s W[d][s], r = (target.max_conc / estimate.max_conc, 0)"""
    target = StainTarget() if target is None else target
    W = torch.linalg.inv(torch.as_tensor(estimate.matrix, dtype=torch.float64).cpu())
    ratio = torch.zeros(3, dtype=torch.float64)
    ratio[:2] = target.max_conc / torch.as_tensor(estimate.max_conc, dtype=torch.float64).cpu()
    return target.matrix.T @ torch.diag(ratio) @ W.T


def normalizer(estimate, target=None, T=MAX_TONE, device=None):
    """(lut int32 (3, 3, 256), tone uint8 (T,)) of ops.stain_apply that recolour a slide of `estimate`'s stains to `target`'s"""
    return apply_lut(transfer_matrix(estimate, target), T, device), tone_table(T, device)


def normalize_slide(slide, estimate=None, target=None, out=None, **estimate_args):
    """The slide recoloured to `target` (default StainTarget()): the estimate is made when none is given (estimate_stains(slide,
    **estimate_args)), then one ops.stain_apply over the whole slide into `out` (None: a new slide; the slide itself: in place)."""
    from . import ops
    if estimate is None:
        estimate = estimate_stains(slide, target=target, **estimate_args)
    lut, tone = normalizer(estimate, target, device=slide.device)
    return ops.stain_apply(slide, lut, tone, out)


def angle_between(a, b):
    """degrees between two vectors"""
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    return math.degrees(math.acos(max(-1.0, min(1.0, float(a @ b) / float(a.norm() * b.norm())))))
