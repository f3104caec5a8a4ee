"""CPU restatement of csrc/paste.hip (a helper next to augment_ref.py and score_ref.py, not a test): the formulas of include/hdyolo.h, 'mask
paste', in numpy fp32.  Every product, sum and quotient is one numpy operation on float32 arrays (numpy never contracts), so it reproduces the
kernels bit for bit: dense mode (torchvision's paste_masks_in_image), the label map of a canvas window, and the areas."""
import numpy as np

f32 = np.float32
COORD_LIMIT = f32(2.0 ** 30)


def ellipse_patch(rng, P=30):
    """test input: sigmoid of a soft ellipse, the shape of a nucleus mask probability, values on both sides of 0.5 (rng: np.random.Generator)"""
    yy, xx = np.mgrid[0:P, 0:P].astype(np.float64)
    cx, cy = rng.uniform(P * 0.3, P * 0.7, 2)
    ax, ay = rng.uniform(P * 0.15, P * 0.5, 2)
    th = rng.uniform(0, np.pi)
    u = (xx - cx) * np.cos(th) + (yy - cy) * np.sin(th)
    v = -(xx - cx) * np.sin(th) + (yy - cy) * np.cos(th)
    return (1.0 / (1.0 + np.exp(-rng.uniform(2, 12) * (1.0 - np.sqrt((u / ax) ** 2 + (v / ay) ** 2))))).astype(f32)


def box_for(bx1, by1, w, h, M, padding=1):
    """test input: an xyxy box whose expansion lands half a pixel inside the integer box [bx1, bx1 + w) x [by1, by1 + h) (w, h >= 1), so that
    no rounding of the expansion can move an edge"""
    scale = (M + 2 * padding) / M
    ex1, ex2, ey1, ey2 = bx1 + 0.5, bx1 + w - 0.5, by1 + 0.5, by1 + h - 0.5
    if bx1 < 0:
        ex1 -= 1.0                   # truncation toward zero: -3.5 -> -3
    if bx1 + w - 1 < 0:
        ex2 -= 1.0
    if by1 < 0:
        ey1 -= 1.0
    if by1 + h - 1 < 0:
        ey2 -= 1.0
    cx, hx, cy, hy = (ex1 + ex2) / 2, (ex2 - ex1) / 2 / scale, (ey1 + ey2) / 2, (ey2 - ey1) / 2 / scale
    return [cx - hx, cy - hy, cx + hx, cy + hy]


def integer_boxes(boxes, M, padding=1):
    """(R, 4) xyxy -> int64 (R, 4) expanded boxes truncated toward zero, and a bool (R,) 'pastes at all' (finite, below 2^30 in magnitude)"""
    b = np.asarray(boxes, dtype=f32).reshape(-1, 4)
    P = M + 2 * padding
    scale = f32(P) / f32(M)
    with np.errstate(all='ignore'):
        hx = ((b[:, 2] - b[:, 0]) * f32(0.5)) * scale
        cx = (b[:, 2] + b[:, 0]) * f32(0.5)
        hy = ((b[:, 3] - b[:, 1]) * f32(0.5)) * scale
        cy = (b[:, 3] + b[:, 1]) * f32(0.5)
        e = np.stack([cx - hx, cy - hy, cx + hx, cy + hy], 1).astype(f32)
        ok = (np.abs(e) < COORD_LIMIT).all(1)                    # NaN compares false
    return np.trunc(np.where(ok[:, None], e, 0)).astype(np.int64), ok


def axis_table(P, n):
    """destination offsets 0 .. n - 1 of an axis resized from P to n: (i0, i1, l0, l1)"""
    sc = f32(P) / f32(n)
    d = np.arange(n).astype(f32)
    s = np.maximum(sc * (d + f32(0.5)) - f32(0.5), f32(0))
    i0 = np.minimum(s.astype(np.int64), P - 1)
    i1 = i0 + (i0 < P - 1)
    l1 = s - i0.astype(f32)
    l0 = f32(1) - l1
    return i0, i1, l0.astype(f32), l1.astype(f32)


def resize(patch, h, w, rows=None, cols=None):
    """patch (P, P) fp32 -> (h, w) bilinear, align_corners=False; rows / cols: slices of the destination to compute (default all)"""
    patch = np.asarray(patch, dtype=f32)
    P = patch.shape[0]
    iy0, iy1, ly0, ly1 = (t[rows if rows is not None else slice(None)] for t in axis_table(P, h))
    ix0, ix1, lx0, lx1 = (t[cols if cols is not None else slice(None)] for t in axis_table(P, w))
    top = lx0[None] * patch[iy0][:, ix0] + lx1[None] * patch[iy0][:, ix1]
    bot = lx0[None] * patch[iy1][:, ix0] + lx1[None] * patch[iy1][:, ix1]
    return (ly0[:, None] * top + ly1[:, None] * bot).astype(f32)


def framed(mask, padding):
    return np.pad(np.asarray(mask, dtype=f32), padding) if padding else np.asarray(mask, dtype=f32)


def pieces(masks, boxes, window, padding=1):
    """yields (row, y slice, x slice, values) of every row's resized patch clipped to window = (x0, y0, w, h); slices index the window"""
    masks = np.asarray(masks, dtype=f32)
    masks = masks.reshape(-1, masks.shape[-2], masks.shape[-1])
    M = masks.shape[-1]
    x0, y0, w, h = window
    ib, ok = integer_boxes(boxes, M, padding)
    for r in range(len(masks)):
        if not ok[r]:
            continue
        bx1, by1, bx2, by2 = (int(v) for v in ib[r])
        bw, bh = max(bx2 - bx1 + 1, 1), max(by2 - by1 + 1, 1)
        cx0, cx1 = max(bx1, x0), min(bx1 + bw, x0 + w)
        cy0, cy1 = max(by1, y0), min(by1 + bh, y0 + h)
        if cx0 >= cx1 or cy0 >= cy1:
            continue
        v = resize(framed(masks[r], padding), bh, bw, slice(cy0 - by1, cy1 - by1), slice(cx0 - bx1, cx1 - bx1))
        yield r, slice(cy0 - y0, cy1 - y0), slice(cx0 - x0, cx1 - x0), v


def paste_masks(masks, boxes, size, padding=1):
    """dense mode: (R, H, W) fp32"""
    H, W = size
    R = len(np.asarray(boxes).reshape(-1, 4))
    out = np.zeros((R, H, W), dtype=f32)
    for r, ys, xs, v in pieces(masks, boxes, (0, 0, W, H), padding):
        out[r, ys, xs] = v
    return out


def label_map(masks, boxes, window, threshold=0.5, padding=1):
    """int32 (h, w) map of window = (x0, y0, w, h): -1 background, else the lowest row whose value is >= threshold"""
    x0, y0, w, h = window
    out = np.full((h, w), -1, dtype=np.int32)
    thr = f32(threshold)
    for r, ys, xs, v in pieces(masks, boxes, window, padding):        # ascending rows: the first owner stays
        sub = out[ys, xs]
        sub[(v >= thr) & (sub < 0)] = r
    return out


def areas(lmap, R):
    lmap = np.asarray(lmap).reshape(-1)
    return np.bincount(lmap[(lmap >= 0) & (lmap < R)], minlength=R).astype(np.int32)[:R]
