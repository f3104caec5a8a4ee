"""Float64 restatement of csrc/roi.hip's RoIAlign family (hdy_roi_align_fwd, hdy_roi_align_bwd, hdy_roi_align_levels_fwd) in plain numpy: no
torch ops, no autograd.  tests/test_roi_ref_host.py pins it to oracle/mask_ref.roi_align under float64 autograd at 1e-12;
tests/test_gpu_roi_direct.py compares the kernels with it.

Layouts: features [B, H, W, C], rois [R, 5] = (image, x1, y1, x2, y2) fp32, output [R, P, P, C], gradient image [B, H, W, C] fp32.

Semantics (torchvision.ops.roi_align as roi.hip documents it).  o = x1 scale - off (off = 0.5 when `aligned`), w = x2 scale - off - o, in
legacy mode max(w, 1); bin = w / P; sample i of bin p lies at o + p bin + (i + 0.5) bin / S.  A sample outside [-1, size] on either axis is
skipped; -1 and size themselves are valid.  A valid coordinate is clamped at 0; at or beyond size - 1 the last row / column interpolates with
itself (weight 1, 0).  A bin is the sum of its S^2 bilinear samples times 1 / S^2; the backward is the transpose, added to `into`.  An image
index outside [0, B) gives zeros (forward) and nothing (backward).

The roi arithmetic is evaluated twice from the same fp32 inputs: `geometry(..., np.float64)` feeds every expected value; `geometry(...,
np.float32)` repeats the kernel's expressions operation for operation (the library is built with -ffp-contract=off) and is used only to
classify cases (which path a roi takes, whether a stored roi has the rounding property it is stored for), never for an expected value.

Bounds, first order in U = 2^-24, from the reference and the launch geometry alone; no element is excluded.
  Coordinate.  With a1 = |x1 scale|, a2 = |x2 scale|, t = x2 scale - off:
      e(o) = U (a1 + |o|),   e(w) = U (a2 + |t|) + e(o) + U |w|   (the clamp at 1 is 1-Lipschitz),   e(bin) = e(w) / P + U |bin|
      d = e(o) + P e(bin) + U P |bin| + 2 U (|o| + P |bin|) + e(bin) + 3 U |bin|
  bounds every sample coordinate of the axis: p bin (p e(bin) + U p |bin|), the sum, (i + .5) bin / S (e(bin) + 2 U |bin|, the factor is
  below 1), the last sum.  v - i0 is exact; 1 - l and the products of two axis weights are charged to the blend below.
  Forward.  The bilinear form is continuous across cell boundaries (and across the clamps at 0 and size - 1), so a coordinate error dy
  costs dy times the slope of the cell: hx |f[i1, x0] - f[i0, x0]| + lx |f[i1, x1] - f[i0, x1]|, 0 in a clamped region; where the sample is
  within dy of an integer the fp32 sample may sit in the neighbouring cell and the largest slope of the cells i0 - 1 .. i0 + 1 is taken.
  The blend: weights 3U, four products U, three sums, S^2 accumulations, 1 / S^2 (2U when S^2 is no power of two): (4 S^2 + 6) U of
  SUM |w f| / S^2, the "4 S^2 terms".
  Backward.  A pixel receives d w_y(h) w_x(w) / S^2 from a sample; dy moves dy |d| w_x / S^2 of it between the rows i0, i1 (i0 - 1 ..
  i1 + 1 where the sample is within dy of an integer; nothing in a clamped region away from an integer), likewise dx.  Roundings inside one
  roi: tiled path d / S^2 (U), a table entry of 2S terms, two sums over P terms, the products: (2P + 2S + 8) U of A = SUM |d| w_y w_x / S^2;
  the scatter path's 6U per term is below that.  Across rois: one fp32 atomic add per contributing roi on the tiled path, one per
  neighbour of a valid sample on the scatter path, in any order, one more for `into`: K U (SUM_r A_r + |into|) with K the number of adds.
  `tiled` (per roi, from roi_cases.classify) only selects which count is charged; without it every roi is charged the scatter count.
  bf16 outputs get 2^-8 (|ref| + bound) on top (segk_ref.finish).
Validity thresholds.  The value is discontinuous only where a sample crosses -1 or size.  `kink_distance` returns how far, in units of its
coordinate bound, the nearest sample of a case lies from them; the host test asserts KINK_MARGIN for every case but the dyadic one, whose
fp32 and fp64 coordinates it asserts equal.  A condition on the inputs, asserted on the CPU; no element is excused.

Non-finite values.  The forward multiplies all four neighbours of a valid sample by their weights, as the kernel does, so a zero weight does
not shield a NaN (0 NaN = NaN, 0 inf = NaN); a skipped sample reads nothing.  `check` (segk_ref) then demands NaN exactly where the reference
has it and the same infinities.  In the backward a non-finite dout reaches the four neighbours of every valid sample of its bin on the
scatter path (what `roi_align_bwd` computes) and the roi's whole footprint on the tiled path (D Wx and Wy^T T multiply it by zero weights):
`check_bwd` demands a non-finite value at least wherever the reference has one, none outside `footprint_mask` of the rois that carry one,
and the bound on every element where both are finite; an element inside such a footprint must be non-finite or within its bound.
"""
import numpy as np

from segk_ref import SLACK, U, check, f64, finish, ratios  # noqa: F401

KINK_MARGIN = 64.0


# ------------------------------------------------------------------------------------------ geometry
def geometry(rois, scale, P, S, aligned, dtype=np.float64):
    """per roi: image index b [R], origins / bins (x0, y0, bin_w, bin_h) [R] and the sample coordinates xs, ys [R, P * S], every operation
    rounded to `dtype` in the kernel's order (roi_geom, roi_bin)"""
    T = dtype
    rois = np.asarray(rois, np.float32).reshape(-1, 5)
    r = rois.astype(T)
    s, off = T(np.float32(scale)), T(0.5 if aligned else 0.0)
    with np.errstate(all='ignore'):
        b = rois[:, 0].astype(np.int64)
        g = dict(b=b)
        for ax, lo, hi in (('x', 1, 3), ('y', 2, 4)):
            o = (r[:, lo] * s - off).astype(T)
            w = ((r[:, hi] * s).astype(T) - off - o).astype(T)
            if not aligned:
                w = np.maximum(w, T(1.0))
            bs = (w / T(P)).astype(T)
            p = np.repeat(np.arange(P), S).astype(T)[None]
            i = np.tile(np.arange(S), P).astype(T)[None]
            v = ((o[:, None] + p * bs[:, None]).astype(T) + (((i + T(0.5)) * bs[:, None]).astype(T) / T(S)).astype(T)).astype(T)
            assert v.dtype == T and bs.dtype == T and o.dtype == T
            g[ax + '0'], g['bin_' + ('w' if ax == 'x' else 'h')], g[ax + 's'] = o, bs, v
    return g


def axis_sample(v, size):
    """torchvision's bilinear setup along one axis (roi.hip axis_sample / sample_at): (ok, i0, i1, lo, hi), weights in v's dtype"""
    T = v.dtype.type
    with np.errstate(all='ignore'):
        ok = ~((v < T(-1.0)) | (v > T(size)))
        v = np.where(v <= 0, T(0.0), v)
        i0 = np.where(np.isfinite(v), v, 0).astype(np.int64)
        edge = i0 >= size - 1
        i0 = np.where(edge, size - 1, i0)
        i1 = np.where(edge, i0, i0 + 1)
        v = np.where(edge, i0.astype(T), v)
        hi = (v - i0.astype(T)).astype(T)
        lo = (T(1.0) - hi).astype(T)
    return ok, i0, i1, lo, hi


def coord_error(rois, scale, P, aligned):
    """(dx [R], dy [R]): the bound of every fp32 sample coordinate's error (module docstring)"""
    r = f64(np.asarray(rois, np.float32).reshape(-1, 5))
    s, off = float(np.float32(scale)), 0.5 if aligned else 0.0
    out = []
    for lo, hi in ((1, 3), (2, 4)):
        a1, a2 = np.abs(r[:, lo] * s), np.abs(r[:, hi] * s)
        o, t = r[:, lo] * s - off, r[:, hi] * s - off
        w = t - o
        if not aligned:
            w = np.maximum(w, 1.0)
        w, bs = np.abs(w), np.abs(w) / P
        eo = U * (a1 + np.abs(o))
        ew = U * (a2 + np.abs(t)) + eo + U * w
        eb = ew / P + U * bs
        out.append(eo + P * eb + U * P * bs + 2 * U * (np.abs(o) + P * bs) + eb + 3 * U * bs)
    return out[0], out[1]


def kink_distance(rois, scale, P, S, aligned, H, W, per_roi=False):
    """the smallest distance of a sample from a validity threshold (-1, size) over the case (or per roi), in units of the sample's
    coordinate bound"""
    g = geometry(rois, scale, P, S, aligned)
    dx, dy = coord_error(rois, scale, P, aligned)
    worst = np.full(len(dx), np.inf)
    for v, d, size in ((g['xs'], dx, W), (g['ys'], dy, H)):
        worst = np.minimum(worst, (np.minimum(np.abs(v + 1.0), np.abs(v - size)) / d[:, None]).min(1))
    return worst if per_roi else float(worst.min()) if len(worst) else np.inf


# ------------------------------------------------------------------------------------------ forward
def _axis_tables(v, d, size):
    """per roi and sample of one axis: ok, i0, i1, lo, hi, near (within d of an integer), inside (not clamped)"""
    ok, i0, i1, lo, hi = axis_sample(v, size)
    near = np.abs(v - np.rint(v)) <= d[:, None]
    inside = (v > 0) & (v < size - 1)
    return ok, i0, i1, lo, hi, near, inside


def _slopes(f, axis):
    """|f[i + 1] - f[i]| along axis 0 or 1 of [H, W, C], one entry per index i (0 for the last) -> (narrow, wide): the cell's own slope and
    the largest of the cells i - 1 .. i + 1"""
    with np.errstate(all='ignore'):
        d = np.abs(np.diff(f, axis=axis))
    d = np.where(np.isfinite(d), d, 0.0)
    z = np.zeros_like(np.take(f, [0], axis=axis))
    nar = np.concatenate([d, z], axis)
    left = np.concatenate([z, nar], axis)
    right = np.concatenate([nar, z], axis)
    n = f.shape[axis]
    sl = lambda a, k: np.take(a, np.arange(k, k + n), axis=axis)        # noqa: E731
    return nar, np.maximum(np.maximum(sl(left, 0), nar), sl(right, 1))


def roi_align_fwd(feat, rois, scale, P, S, aligned, with_bound=False):
    """feat [B, H, W, C] -> out [R, P, P, C] (and its fp32 bound)"""
    feat = f64(feat)
    B, H, W, C = feat.shape
    rois = np.asarray(rois, np.float32).reshape(-1, 5)
    R = rois.shape[0]
    g = geometry(rois, scale, P, S, aligned)
    dx, dy = coord_error(rois, scale, P, aligned)
    oky, y0, y1, ly0, ly1, ny, iny = _axis_tables(g['ys'], dy, H)
    okx, x0, x1, lx0, lx1, nx, inx = _axis_tables(g['xs'], dx, W)
    out, bound = np.zeros((R, P, P, C)), np.zeros((R, P, P, C))
    slopes = {}
    for r in range(R):
        b = int(g['b'][r])
        if not 0 <= b < B:
            continue
        f = feat[b]
        ok = (oky[r][:, None] & okx[r][None, :])[..., None]
        wy0, wy1, wx0, wx1 = ly0[r][:, None, None], ly1[r][:, None, None], lx0[r][None, :, None], lx1[r][None, :, None]
        a, bb, c, d = f[y0[r]][:, x0[r]], f[y0[r]][:, x1[r]], f[y1[r]][:, x0[r]], f[y1[r]][:, x1[r]]
        with np.errstate(all='ignore'):
            v = (wy0 * wx0) * a + (wy0 * wx1) * bb + (wy1 * wx0) * c + (wy1 * wx1) * d
            v = np.where(ok, v, 0.0)
            out[r] = v.reshape(P, S, P, S, C).sum((1, 3)) / (S * S)
        if not with_bound:
            continue
        if b not in slopes:
            slopes[b] = (_slopes(f, 0), _slopes(f, 1))
        (ny_, wy_), (nx_, wx_) = slopes[b]
        with np.errstate(all='ignore'):
            fin = lambda t: np.where(np.isfinite(t), np.abs(t), 0.0)                           # noqa: E731
            mag = (wy0 * wx0) * fin(a) + (wy0 * wx1) * fin(bb) + (wy1 * wx0) * fin(c) + (wy1 * wx1) * fin(d)
            # slope along y at the sample: the cell's own where it is inside the map and away from an integer, the widest of three cells near one
            sy = np.where(ny[r][:, None, None], wx0 * wy_[y0[r]][:, x0[r]] + wx1 * wy_[y0[r]][:, x1[r]],
                          np.where(iny[r][:, None, None], wx0 * ny_[y0[r]][:, x0[r]] + wx1 * ny_[y0[r]][:, x1[r]], 0.0))
            sx = np.where(nx[r][None, :, None], wy0 * wx_[y0[r]][:, x0[r]] + wy1 * wx_[y1[r]][:, x0[r]],
                          np.where(inx[r][None, :, None], wy0 * nx_[y0[r]][:, x0[r]] + wy1 * nx_[y1[r]][:, x0[r]], 0.0))
            e = np.where(ok, dy[r] * sy + dx[r] * sx + (4 * S * S + 6) * U * mag, 0.0)
            bound[r] = e.reshape(P, S, P, S, C).sum((1, 3)) / (S * S)
    return (out, bound) if with_bound else out


# ------------------------------------------------------------------------------------------ backward
def _weight_rows(ok, i0, i1, lo, hi, near, inside, d, size, P, S):
    """one roi, one axis -> (Wt [P, size] the summed weights, A [P, size] their magnitudes, E [P, size] the weight that a coordinate error
    can move onto each index, N [P, size] the number of (sample, neighbour) pairs that touch it)"""
    Wt, E, N = np.zeros((P, size)), np.zeros((P, size)), np.zeros((P, size))
    for k in range(P * S):
        if not ok[k]:
            continue
        p = k // S
        Wt[p, i0[k]] += lo[k]
        Wt[p, i1[k]] += hi[k]
        N[p, i0[k]] += 1
        N[p, i1[k]] += 1
        if near[k]:
            E[p, max(i0[k] - 1, 0):min(i1[k] + 1, size - 1) + 1] += d
        elif inside[k]:
            E[p, i0[k]] += d
            E[p, i1[k]] += d
    return Wt, np.abs(Wt), E, N


def _roi_axes(rois, scale, P, S, aligned, H, W):
    g = geometry(rois, scale, P, S, aligned)
    dx, dy = coord_error(rois, scale, P, aligned)
    ty, tx = _axis_tables(g['ys'], dy, H), _axis_tables(g['xs'], dx, W)
    for r in range(len(g['b'])):
        yield r, int(g['b'][r]), _weight_rows(*(t[r] for t in ty), dy[r], H, P, S), _weight_rows(*(t[r] for t in tx), dx[r], W, P, S)


def _sep(D, My, Mx):
    """SUM_pq D[p, q, c] My[p, h] Mx[q, w] -> [h, w, c]"""
    return np.moveaxis(np.tensordot(np.tensordot(My, D, axes=(0, 0)), Mx, axes=(1, 0)), 2, 1)


def roi_align_bwd(dout, shape, rois, scale, S, aligned, into=None, with_bound=False, tiled=None):
    """dout [R, P, P, C] -> the gradient image [B, H, W, C] (added to `into`), and its fp32 bound.  A non-finite dout reaches the four
    neighbours of every valid sample of its bin, whatever their weights (the scatter path's pattern)."""
    dout = f64(dout)
    B, H, W, C = shape
    R, P = dout.shape[:2]
    img = np.zeros((B, H, W, C)) if into is None else f64(into).copy()
    A = np.zeros((B, H, W, C))
    mov = np.zeros((B, H, W, C))
    K = np.zeros((B, H, W, 1)) + (0 if into is None else 1)
    bad = ~np.isfinite(dout)
    D = np.where(bad, 0.0, dout) / (S * S)
    for r, b, (Wy, Ay, Ey, Ny), (Wx, Ax, Ex, Nx) in _roi_axes(rois, scale, P, S, aligned, H, W):
        if not 0 <= b < B:
            continue
        img[b] += _sep(D[r], Wy, Wx)
        if bad[r].any():
            touched = _sep(bad[r].astype(np.float64), Ny, Nx) > 0
            img[b] = np.where(touched, np.nan, img[b])
        if with_bound:
            a = np.abs(D[r])
            Ar = _sep(a, Ay, Ax)
            A[b] += Ar
            mov[b] += _sep(a, Ey, Ax) + _sep(a, Ay, Ex) + (2 * P + 2 * S + 8) * U * Ar
            n = np.einsum('ph,qw->hw', Ny.sum(0, keepdims=True), Nx.sum(0, keepdims=True))
            hit = n > 0
            K[b, ..., 0] += np.where(hit, 1.0, 0.0) if (tiled is not None and tiled[r]) else np.einsum('ph,qw->hw', Ny, Nx)
    if not with_bound:
        return img
    old = 0.0 if into is None else np.abs(f64(into))
    return img, SLACK * (mov + K * U * (A + old))


def footprint_mask(shape, rois, scale, P, S, aligned, which):
    """[B, H, W, C] bool: the footprint (rows and columns between the smallest i0 and the largest i1 of the valid samples) of every roi r with
    which[r] [C] set, on those channels"""
    B, H, W, C = shape
    m = np.zeros(shape, bool)
    for r, b, (_, _, _, Ny), (_, _, _, Nx) in _roi_axes(rois, scale, P, S, aligned, H, W):
        hs, ws = np.nonzero(Ny.sum(0))[0], np.nonzero(Nx.sum(0))[0]
        if 0 <= b < B and which[r].any() and len(hs) and len(ws):
            m[b, hs.min():hs.max() + 1, ws.min():ws.max() + 1, which[r]] = True
    return m


def cover_count(shape, rois, scale, P, S, aligned):
    """[B, H, W]: how many rois have the pixel inside their footprint"""
    return sum(footprint_mask(shape[:3] + (1,), rois[r:r + 1], scale, P, S, aligned, np.ones((1, 1), bool))[..., 0].astype(np.int64)
               for r in range(len(rois)))


def check_bwd(got, ref, bound, may, what=''):
    """the backward's comparer where dout holds non-finite values: got is non-finite wherever `ref` is, finite outside `may`, and within the
    bound wherever both are finite (inside `may` an element is non-finite or within its bound); returns the worst error / bound"""
    got, ref = f64(got), f64(ref)
    gbad, rbad = ~np.isfinite(got), ~np.isfinite(ref)
    assert (gbad | ~rbad).all(), f'{what}: {int((rbad & ~gbad).sum())} elements are finite where the reference is not'
    assert not (gbad & ~may & ~rbad).any(), f'{what}: {int((gbad & ~may & ~rbad).sum())} non-finite elements outside the footprints that may hold one'
    assert rbad[may].any() or not may.any(), f'{what}: the reference holds no non-finite value'
    return check(np.where(gbad, 0.0, got), np.where(gbad, 0.0, ref), np.where(rbad, 1.0, bound), what)


# ------------------------------------------------------------------------------------------ multi-level
def compact_rows(n_keep, max_det, out_rows):
    """(image, padded slot) of every compacted row the launch writes: n_keep clamped to [0, max_det], the first min(out_rows, total)"""
    n = np.clip(np.asarray(n_keep, np.int64), 0, max_det)
    rows = [(b, j) for b in range(len(n)) for j in range(int(n[b]))]
    return rows[:min(int(out_rows), len(rows))], len(rows)


def roi_align_levels(feats, scales, boxes, level, n_keep, out_rows, P, S, aligned, prefill):
    """feats: per level [B, H, W, C]; boxes [B, max_det, 4] fp32, level [B, max_det], n_keep [B] -> (out [out_rows, P, P, C], bound, written
    rows): a row whose level is not finite or outside (-1, levels) is zeros, rows at or behind min(out_rows, total) keep `prefill`"""
    boxes, level = np.asarray(boxes, np.float32), np.asarray(level, np.float32)
    B, max_det = boxes.shape[:2]
    C = feats[0].shape[3]
    rows, _ = compact_rows(n_keep, max_det, out_rows)
    out = np.full((int(out_rows), P, P, C), float(prefill))
    bound = np.zeros_like(out)
    out[:len(rows)] = 0.0
    with np.errstate(all='ignore'):
        lv = [int(level[b, j]) if (level[b, j] > -1.0 and level[b, j] < len(feats)) else -1 for b, j in rows]
    for l in range(len(feats)):
        sel = [k for k, v in enumerate(lv) if v == l]
        if sel:
            rois = np.array([[rows[k][0], *boxes[rows[k]]] for k in sel], np.float32)
            o, bd = roi_align_fwd(feats[l], rois, scales[l], P, S, aligned, with_bound=True)
            out[sel], bound[sel] = o, bd
    return out, bound, len(rows)
