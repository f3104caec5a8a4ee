"""Texture of a nucleus: from the level counts of ops.label_texture (hdy_label_texture, include/hdyolo_texture.h) to table columns.

The pass counts; this module makes the table the pass reads (stain_lut) and turns its counts into features (intensity, haralick,
texture_table).  Like measure.nucleus_table, intensity and haralick are tensor arithmetic on whole arrays of counts: float64 operations
without a loop over rows or a read of a value, on whatever device the counts live (the GPU in the slide path, the CPU in the tests).  Every
reduction is a plain `sum` over a fixed shape, no scatter and no atomic, so the same counts give the same bits.

stain_lut.  The pass adds three table entries and shifts: level = clamp((lut[0][R] + lut[1][G] + lut[2][B]) >> 16, 0, levels - 1).  For a
stain the table holds colour deconvolution (Ruifrok and Johnston 2001): the optical density of a channel value v is od(v) = -log10((v + 1)
/ 256), the rows of the stain matrix M are the unit optical-density vectors of the stains, and the concentration of stain s in a pixel is
sum_c W[c][s] od(v_c) with W = inverse(M).  Entry [c][v] = round(2^16 levels W[c][s] od(v) / od_max) in float64, so that the pass's level is
floor(levels * concentration / od_max) clamped: od_max is the concentration that reaches the top level.  Three entries, each rounded by at
most half a unit of 2^-16, move the quantity by at most 1.5 * 2^-16 of a level: a colour whose exact value lies farther than that from an
integer gets the exact level.

haralick.  The 13 features of Haralick, Shanmugam and Dinstein (1973) per direction, levels indexed 0 .. L - 1, natural logarithms with
0 log 0 = 0, p = glcm / sum(glcm), px / py its row / column sums, mx, my, sx, sy their means and standard deviations, p+(k) the distribution
of i + j (k = 0 .. 2L - 2), p-(k) that of |i - j| (k = 0 .. L - 1).  Variances and the correlation numerator are formed about the mean
(centred), not as a difference of large sums:
     0 asm                  sum p^2
     1 contrast             sum (i - j)^2 p
     2 correlation          sum (i - mx) (j - my) p / (sx sy);  1 where sx sy = 0 (a single level)
     3 variance             sum (i - mx)^2 p
     4 idm                  sum p / (1 + (i - j)^2)
     5 sum_average          sum k p+(k)
     6 sum_variance         sum (k - sum_average)^2 p+(k)
     7 sum_entropy          -sum p+ log p+
     8 entropy              HXY = -sum p log p
     9 difference_variance  the variance of p-
    10 difference_entropy   -sum p- log p-
    11 imc1                 (HXY - HXY1) / max(HX, HY) with HXY1 = -sum p log(px py);  0 where max(HX, HY) = 0
    12 imc2                 sqrt(max(1 - exp(-2 (HXY2 - HXY)), 0)) with HXY2 = -sum px py log(px py)
A direction without pairs (sum(glcm) = 0: a single pixel, a flagged label) gives NaN in all 13.
"""
import torch

from . import _ext

FEATURES = ('asm', 'contrast', 'correlation', 'variance', 'idm', 'sum_average', 'sum_variance', 'sum_entropy', 'entropy', 'difference_variance',
            'difference_entropy', 'imc1', 'imc2')
INTENSITY = ('level_mean', 'level_std', 'level_skewness', 'level_kurtosis', 'level_entropy', 'level_min', 'level_median', 'level_max')
OFFSETS = ((0, 1), (-1, 1), (-1, 0), (-1, -1))                # (di, dj): 0, 45, 90 and 135 degrees at distance 1
SHIFT = _ext.CONSTANTS['HDY_TEXTURE_SHIFT']
ENTRY_BOUND = 1 << 28                                         # three entries below it cannot wrap the pass's 32-bit sum
RUIFROK_H, RUIFROK_E = (0.65, 0.70, 0.29), (0.07, 0.99, 0.11)
REC601 = (0.299, 0.587, 0.114)
# the concentration that reaches the top level.  A choice, not a measurement: haematoxylin of a dense nucleus reaches about 2 units of optical
# density, eosin and the residual stay lower.  For 'gray' / 'r' / 'g' / 'b' the quantity is a pixel value and the bound is 256.
OD_MAX = {'hematoxylin': 2.0, 'eosin': 1.5, 'residual': 1.5, 'gray': 256.0, 'r': 256.0, 'g': 256.0, 'b': 256.0}


def stain_matrix():
    """float64 (3, 3): the unit optical-density vectors of haematoxylin and eosin (Ruifrok-Johnston) and their unit cross product"""
    h = torch.tensor(RUIFROK_H, dtype=torch.float64)
    e = torch.tensor(RUIFROK_E, dtype=torch.float64)
    h, e = h / h.norm(), e / e.norm()
    r = torch.linalg.cross(h, e)
    return torch.stack([h, e, r / r.norm()])


def stain_weights(stain='hematoxylin', od_max=None, matrix=None):
    """(coef float64 (3,), value float64 (256,), od_max): the pass's quantity for `stain` is sum_c coef[c] * value[v_c], and od_max reaches the
    top level.  For a stain: column s of inverse(matrix) and the optical density; for 'gray' / 'r' / 'g' / 'b': weights of the pixel value."""
    if stain not in OD_MAX:
        raise ValueError(f'stain_lut: unknown stain {stain!r} (one of {", ".join(OD_MAX)})')
    od_max = float(OD_MAX[stain] if od_max is None else od_max)
    if not od_max > 0:
        raise ValueError(f'stain_lut: od_max={od_max} must be positive')
    v = torch.arange(256, dtype=torch.float64)
    if stain in ('hematoxylin', 'eosin', 'residual'):
        m = stain_matrix() if matrix is None else torch.as_tensor(matrix, dtype=torch.float64).cpu()
        if tuple(m.shape) != (3, 3):
            raise ValueError(f'stain_lut: the stain matrix must be 3 x 3 (rows = stains), got {tuple(m.shape)}')
        coef = torch.linalg.inv(m)[:, ('hematoxylin', 'eosin', 'residual').index(stain)]
        return coef, -torch.log10((v + 1) / 256), od_max
    coef = torch.tensor(REC601 if stain == 'gray' else [float(stain == c) for c in 'rgb'], dtype=torch.float64)
    return coef, v, od_max


def stain_lut(stain='hematoxylin', levels=16, od_max=None, matrix=None, device=None):
    """int32 (3, 256): the table of ops.label_texture for `stain` at `levels` levels (module docstring).  stain: 'hematoxylin', 'eosin',
    'residual' (colour deconvolution with `matrix`, rows = unit optical-density vectors of the three stains, default Ruifrok-Johnston),
    'gray' (Rec. 601 luma) or 'r' / 'g' / 'b' (one channel).  od_max: the value that reaches the top level; the defaults (2.0 for haematoxylin,
    1.5 for eosin and the residual, 256 for pixel values) are a choice.  A table with an entry of magnitude 2^28 or more is refused: the
    pass's 32-bit sum of three entries must not wrap."""
    levels = int(levels)
    if levels not in (8, 16, 32):
        raise ValueError(f'stain_lut: levels={levels} (8, 16 or 32)')
    coef, value, od_max = stain_weights(stain, od_max, matrix)
    lut = torch.round((1 << SHIFT) * levels * coef[:, None] * value[None, :] / od_max)
    if not bool(torch.isfinite(lut).all()) or float(lut.abs().max()) >= ENTRY_BOUND:
        raise ValueError(f'stain_lut: an entry reaches 2^28 (stain={stain!r}, levels={levels}, od_max={od_max}): the sum of three would wrap')
    return lut.to(torch.int32).to(device) if device is not None else lut.to(torch.int32)


def _xlogx(p):
    return torch.xlogy(p, p)


def _skew_sum(p):
    """(.., 2L - 1): s[k] = sum of p[i][j] over i + j = k, as one strided view and one sum (no scatter): rows padded to 2L, the flat array read
    as rows of 2L - 1, which moves entry (i, j) to column i + j of row i"""
    L = p.shape[-1]
    flat = torch.nn.functional.pad(p, (0, L)).reshape(*p.shape[:-2], 2 * L * L)
    return flat[..., :L * (2 * L - 1)].reshape(*p.shape[:-2], L, 2 * L - 1).sum(-2)


def haralick(glcm):
    """float64 (n, D, 13) from the counts (n, D, L, L) of ops.label_texture: the 13 Haralick features per direction, in the order of FEATURES
    (module docstring).  Conventions: a direction without pairs gives NaN in all 13; with sx sy = 0 the correlation is 1; with max(HX, HY) = 0
    imc1 is 0; sum_variance is taken about sum_average."""
    if glcm.dim() != 4 or glcm.shape[-1] != glcm.shape[-2]:
        raise ValueError(f'haralick: glcm must be (n, D, L, L), got {tuple(glcm.shape)}')
    f64 = torch.float64
    L = glcm.shape[-1]
    g = glcm.to(f64)
    total = g.sum((-1, -2), keepdim=True)
    p = g / torch.where(total > 0, total, torch.full_like(total, float('nan')))
    lv = torch.arange(L, dtype=f64, device=glcm.device)
    i, j = lv[:, None], lv[None, :]
    px, py = p.sum(-1), p.sum(-2)
    mx, my = (px * lv).sum(-1), (py * lv).sum(-1)
    ci, cj = i - mx[..., None, None], j - my[..., None, None]
    varx = ((lv - mx[..., None]) ** 2 * px).sum(-1)
    vary = ((lv - my[..., None]) ** 2 * py).sum(-1)
    sxy = torch.sqrt(varx) * torch.sqrt(vary)
    cov = (ci * cj * p).sum((-1, -2))
    d2 = (i - j) ** 2
    out = torch.empty((*glcm.shape[:2], 13), dtype=f64, device=glcm.device)
    out[..., 0] = (p * p).sum((-1, -2))
    out[..., 1] = (d2 * p).sum((-1, -2))
    out[..., 2] = torch.where(sxy > 0, cov / sxy, torch.where(torch.isnan(sxy), sxy, torch.ones_like(sxy)))
    out[..., 3] = (ci * ci * p).sum((-1, -2))
    out[..., 4] = (p / (1 + d2)).sum((-1, -2))
    ps = _skew_sum(p)                                                     # p+(k), k = 0 .. 2L - 2
    ks = torch.arange(2 * L - 1, dtype=f64, device=glcm.device)
    savg = (ks * ps).sum(-1)
    out[..., 5] = savg
    out[..., 6] = ((ks - savg[..., None]) ** 2 * ps).sum(-1)
    out[..., 7] = -_xlogx(ps).sum(-1)
    hxy = -_xlogx(p).sum((-1, -2))
    out[..., 8] = hxy
    sd = _skew_sum(p.flip(-1))                                            # sums over i - j = k - (L - 1)
    pd = sd[..., L - 1:].clone()                                          # p-(k), k = 0 .. L - 1
    pd[..., 1:] += sd[..., :L - 1].flip(-1)
    davg = (lv * pd).sum(-1)
    out[..., 9] = ((lv - davg[..., None]) ** 2 * pd).sum(-1)
    out[..., 10] = -_xlogx(pd).sum(-1)
    hx, hy = -_xlogx(px).sum(-1), -_xlogx(py).sum(-1)
    pxy = px[..., :, None] * py[..., None, :]
    hxy1 = -torch.xlogy(p, pxy).sum((-1, -2))
    hxy2 = -_xlogx(pxy).sum((-1, -2))
    hmax = torch.maximum(hx, hy)
    out[..., 11] = torch.where(hmax > 0, (hxy - hxy1) / hmax, torch.where(torch.isnan(hmax), hmax, torch.zeros_like(hmax)))
    out[..., 12] = torch.sqrt(torch.clamp(1 - torch.exp(-2 * (hxy2 - hxy)), min=0))
    return out


def intensity(hist, levels):
    """dict of float64 (n,) columns (INTENSITY) from the level histograms (n, levels) of ops.label_texture: of the distribution of levels
    0 .. levels - 1 over the label's pixels, 'level_mean', 'level_std' (population), 'level_skewness' = m3 / std^3 and 'level_kurtosis' =
    m4 / std^4 (both 0 where std = 0), 'level_entropy' (natural logarithm), 'level_min', 'level_median' (the lowest level at which the
    cumulative count reaches half of the pixels) and 'level_max'.  A label without pixels has NaN in all of them."""
    if hist.dim() != 2 or hist.shape[1] != int(levels):
        raise ValueError(f'intensity: hist must be (n, {int(levels)}), got {tuple(hist.shape)}')
    f64 = torch.float64
    L = hist.shape[1]
    c = hist.to(torch.int64)
    n = c.sum(-1)
    nan = torch.full((hist.shape[0],), float('nan'), dtype=f64, device=hist.device)
    p = c.to(f64) / torch.where(n > 0, n.to(f64), nan)[:, None]
    lv = torch.arange(L, dtype=f64, device=hist.device)
    mean = (p * lv).sum(-1)
    dev = lv[None, :] - mean[:, None]
    m2, m3, m4 = (p * dev ** 2).sum(-1), (p * dev ** 3).sum(-1), (p * dev ** 4).sum(-1)
    std = torch.sqrt(m2)
    flat = lambda v: torch.where(std > 0, v, torch.where(torch.isnan(std), std, torch.zeros_like(std)))      # noqa: E731
    idx = torch.arange(L, dtype=torch.int64, device=hist.device)
    has = c > 0
    some = n > 0
    lo = torch.where(has, idx, L).amin(-1)
    hi = torch.where(has, idx, -1).amax(-1)
    med = (2 * c.cumsum(-1) < n[:, None]).sum(-1)
    col = lambda v: torch.where(some, v.to(f64), nan)                                                        # noqa: E731
    return {'level_mean': mean, 'level_std': std, 'level_skewness': flat(m3 / (m2 * std)), 'level_kurtosis': flat(m4 / (m2 * m2)),
            'level_entropy': -_xlogx(p).sum(-1), 'level_min': col(lo), 'level_median': col(med), 'level_max': col(hi)}


def columns(hist, glcm, flags):
    """the table columns of one chunk of counts: 'tex_<intensity column>', 'tex_<feature>_mean' and 'tex_<feature>_range' over the directions
    that have pairs (NaN where none has), 'tex_flags'; float64 (n,) each"""
    table = {f'tex_{k}': v for k, v in intensity(hist, hist.shape[1]).items()}
    f = haralick(glcm)                                                    # (n, D, 13)
    there = ~torch.isnan(f)
    cnt = there.sum(1)
    zero = torch.zeros_like(f)
    mean = torch.where(there, f, zero).sum(1) / torch.where(cnt > 0, cnt.to(f.dtype), torch.full_like(cnt, float('nan'), dtype=f.dtype))
    big = torch.full_like(f, float('inf'))
    span = torch.where(there, f, -big).amax(1) - torch.where(there, f, big).amin(1)
    span = torch.where(cnt > 0, span, torch.full_like(span, float('nan')))
    for k, name in enumerate(FEATURES):
        table[f'tex_{name}_mean'] = mean[:, k]
        table[f'tex_{name}_range'] = span[:, k]
    table['tex_flags'] = flags.to(torch.float64)
    return table


def texture_table(label_map, R, extent, image, window=(0, 0), stain='hematoxylin', levels=16, offsets=OFFSETS, chunk=16384, matrix=None):
    """dict of float64 (R,) columns of the R labels of an int32 (h, w) label map on the GPU: the INTENSITY columns as 'tex_level_mean', ...,
    for each of the 13 FEATURES its mean and its range (largest minus smallest) over the D directions as 'tex_<feature>_mean' and
    'tex_<feature>_range', and 'tex_flags' (0 measured, 1 the label owns nothing, 2 a box side above 1024).  Directions without pairs are left
    out of the mean and the range; a label none of whose directions has a pair (a single pixel, a flagged label) has NaN there.
    extent, image, window, levels, offsets: as ops.label_texture takes them; stain, matrix: as stain_lut (matrix None: the Ruifrok-Johnston
    vectors; a slide's own, stain.estimate_stains(slide).matrix, measures its stains).  The labels are worked through in chunks
    of `chunk` (ops.label_texture(rows=...)), so that at most chunk * D * levels^2 * 4 bytes of matrices exist at once (64 MB at the defaults).
    Nothing is read back."""
    from . import ops
    R, chunk = int(R), int(chunk)
    if chunk < 1:
        raise ValueError(f'texture_table: chunk={chunk} must be positive')
    dev = label_map.device
    lut = stain_lut(stain, levels, matrix=matrix, device=dev)
    names = [f'tex_{k}' for k in INTENSITY] + [f'tex_{n}_{s}' for n in FEATURES for s in ('mean', 'range')] + ['tex_flags']
    table = {k: torch.empty((R,), dtype=torch.float64, device=dev) for k in names}
    if R == 0:
        ops.label_texture(label_map, R, extent, image, lut, levels, offsets, window, (0, 0))      # the checks of an empty call
    for row0 in range(0, R, chunk):
        n = min(chunk, R - row0)
        part = columns(*ops.label_texture(label_map, R, extent, image, lut, levels, offsets, window, (row0, n)))
        for k in names:
            table[k][row0:row0 + n] = part[k]
    return table
