"""CPU restatement of csrc/augment.hip (a helper next to nms_checker.py, not a test): the formulas of include/hdyolo.h, 'training
augmentation from an 8-bit tile bank', in numpy.  The image side is integer arithmetic behind a handful of fp32 operations, each rounded on
its own (numpy never contracts), so it reproduces the kernel bit for bit; the box side runs in fp32 (the kernel's arithmetic) or in float64
(the reference's, compared with tests/golden/augment.npz)."""
import numpy as np

CELL_BYTES = 864
F_HFLIP, F_VFLIP, F_TRANSPOSE, F_HSV, F_PERSP = 1, 2, 4, 8, 16


def u8_table():
    """v / 255 correctly rounded to fp32 (IEEE division)"""
    return np.arange(256, dtype=np.float32) / np.float32(255)


def parse_cells(cells):
    """uint8 (n, 864) -> dict of per-cell arrays"""
    cells = np.ascontiguousarray(cells)
    w, f = cells[:, :96].view(np.int32), cells[:, :96].view(np.float32)
    return {'src': w[:, 0].copy(), 'Minv': f[:, 1:10].copy(), 'flags': w[:, 10].copy(), 'M': f[:, 11:20].copy(), 'scale': f[:, 20].copy(),
            'lut': cells[:, 96:].reshape(-1, 3, 256).copy()}


def hsv_round_trip(r, g, b, lut):
    """integer arrays r, g, b (any shape) and lut (..., 3, 256) matching their shape -> (r, g, b) after RGB -> HSV -> tables -> RGB"""
    r, g, b = (a.astype(np.int64) for a in (r, g, b))
    V = np.maximum(r, np.maximum(g, b))
    d = V - np.minimum(r, np.minimum(g, b))
    S = np.where(V > 0, (255 * d + (V >> 1)) // np.maximum(V, 1), 0)
    is_r, is_g = V == r, (V == g) & (V != r)
    num = np.where(is_r, g - b, np.where(is_g, b - r, r - g))
    off = np.where(is_r, 0, np.where(is_g, 60, 120))
    d1 = np.maximum(d, 1)
    H = off + (60 * (num + d1) + d1) // (2 * d1) - 30
    H = np.where(H < 0, H + 180, H)
    H = np.where(d > 0, H, 0)
    take = lambda ch, idx: np.take_along_axis(lut[..., ch, :], idx[..., None], -1)[..., 0].astype(np.int64)
    Hn, Sn, Vn = take(0, H), take(1, S), take(2, V)
    Hn = np.where(Hn >= 180, Hn - 180, Hn)
    sec = Hn // 30
    f = Hn - 30 * sec
    p = (Vn * (255 - Sn) + 127) // 255
    q = (Vn * (7650 - Sn * f) + 3825) // 7650
    t = (Vn * (7650 - Sn * (30 - f)) + 3825) // 7650
    R = np.choose(sec, [Vn, q, p, p, t, Vn])
    G = np.choose(sec, [t, Vn, Vn, q, p, p])
    B = np.choose(sec, [p, p, t, Vn, Vn, q])
    return R, G, B


def augment_tiles_ref(tiles, cells, crop, P, k, S, cval):
    """tiles uint8 (n, H, W, 3 | 4) numpy; cells uint8 (B k k, 864); crop int (B, 2) -> uint8 (B, 3, S, S): the byte p of every output pixel
    (the kernel writes table[p] in its dtype)."""
    c = parse_cells(cells)
    n, H, W = tiles.shape[:3]
    B = len(crop)
    out = np.empty((B, 3, S, S), np.uint8)
    f32 = np.float32
    for b in range(B):
        cx, cy = int(crop[b][0]), int(crop[b][1])
        if not (0 <= cx <= k * P - S and 0 <= cy <= k * P - S):
            out[b] = cval
            continue
        X, Y = np.meshgrid(cx + np.arange(S), cy + np.arange(S))
        cc, rr = X // P, Y // P
        ci = (b * k + rr) * k + cc
        flags = c['flags'][ci]
        u, v = X - cc * P, Y - rr * P
        tr = (flags & F_TRANSPOSE) != 0
        u, v = np.where(tr, v, u), np.where(tr, u, v)
        v = np.where(flags & F_VFLIP, P - 1 - v, v)
        u = np.where(flags & F_HFLIP, P - 1 - u, u)
        fu, fv = u.astype(f32), v.astype(f32)
        m = c['Minv'][ci]                                                         # (S, S, 9) fp32
        with np.errstate(all='ignore'):
            sx = (m[..., 0] * fu + m[..., 1] * fv) + m[..., 2]
            sy = (m[..., 3] * fu + m[..., 4] * fv) + m[..., 5]
            sw = (m[..., 6] * fu + m[..., 7] * fv) + m[..., 8]
            persp = (flags & F_PERSP) != 0
            sx = np.where(persp, sx / sw, sx)
            sy = np.where(persp, sy / sw, sy)
            tx, ty = sx * f32(32), sy * f32(32)
            assert tx.dtype == f32 and sx.dtype == f32
            lim = f32(16777216.0)
            ok = (tx >= -lim) & (tx <= lim) & (ty >= -lim) & (ty <= lim)
        qx = np.rint(np.where(ok, tx, 0)).astype(np.int64)
        qy = np.rint(np.where(ok, ty, 0)).astype(np.int64)
        x0, y0, fx, fy = qx >> 5, qy >> 5, qx & 31, qy & 31
        src = c['src'][ci].astype(np.int64)
        ok &= (src >= 0) & (src < n)
        srcc = np.clip(src, 0, n - 1)
        hsv = (flags & F_HSV) != 0
        lut = c['lut'][ci]                                                        # (S, S, 3, 256)
        tex = []
        for j in range(4):
            x, y = x0 + (j & 1), y0 + (j >> 1)
            inside = ok & (x >= 0) & (x < W) & (y >= 0) & (y < H)
            px = tiles[srcc, np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)][..., :3].astype(np.int64)
            R, G, Bc = hsv_round_trip(px[..., 0], px[..., 1], px[..., 2], lut)
            px = np.where(hsv[..., None], np.stack([R, G, Bc], -1), px)
            tex.append(np.where(inside[..., None], px, cval))
        w00, w01, w10, w11 = (32 - fx) * (32 - fy), fx * (32 - fy), (32 - fx) * fy, fx * fy
        p = (tex[0] * w00[..., None] + tex[1] * w01[..., None] + tex[2] * w10[..., None] + tex[3] * w11[..., None] + 512) >> 10
        out[b] = p.transpose(2, 0, 1).astype(np.uint8)
    return out


def warp_box(box, M, scale, flags, r, c, P, S, cx, cy, dt):
    """One cell's boxes (m, 4) through the target pipeline in arithmetic `dt` (np.float32: the kernel's; np.float64: the reference's).
    M: 9 values of that type.  Returns (boxes / S (m, 4), keep (m,) bool, canvas boxes before the flips (m, 4), boxes in output pixels (m, 4))."""
    box = np.asarray(box, dt).reshape(-1, 4)
    M = np.asarray(M, dt).reshape(9)
    sc, fP, fS = dt(scale), dt(P), dt(S)
    xs, ys = box[:, [0, 0, 2, 2]], box[:, [1, 3, 3, 1]]
    with np.errstate(all='ignore'):
        X = (xs * M[0] + ys * M[1]) + M[2]
        Y = (xs * M[3] + ys * M[4]) + M[5]
        if flags & F_PERSP:
            Wd = (xs * M[6] + ys * M[7]) + M[8]
            X, Y = X / Wd, Y / Wd
        X, Y = np.fmin(np.fmax(X, dt(0)), fP), np.fmin(np.fmax(Y, dt(0)), fP)
        nb = np.stack([X.min(1), Y.min(1), X.max(1), Y.max(1)], 1)
        nb[~(X != 0).any(1)] = 0
        canvas = nb.copy()
        eps = dt(1e-16)
        w1, h1 = box[:, 2] * sc - box[:, 0] * sc, box[:, 3] * sc - box[:, 1] * sc
        w2, h2 = nb[:, 2] - nb[:, 0], nb[:, 3] - nb[:, 1]
        ar = np.fmax(w2 / (h2 + eps), h2 / (w2 + eps))
        keep = (w2 > dt(2)) & (h2 > dt(2)) & ((w2 * h2) / (w1 * h1 + eps) > dt(0.1)) & (ar < dt(100))
        x1, y1, x2, y2 = nb.T
        if flags & F_HFLIP:
            x1, x2, y1, y2 = np.abs(x2 - fP), np.abs(x1 - fP), np.abs(y1), np.abs(y2)
        if flags & F_VFLIP:
            y1, y2, x1, x2 = np.abs(y2 - fP), np.abs(y1 - fP), np.abs(x1), np.abs(x2)
        if flags & F_TRANSPOSE:
            x1, y1, x2, y2 = y1, x1, y2, x2
        ox, oy = dt(c * P) - dt(cx), dt(r * P) - dt(cy)
        x1, x2, y1, y2 = x1 + ox, x2 + ox, y1 + oy, y2 + oy
        keep &= (x1 < x2) & (y1 < y2)                         # the crop's filter, on the unclipped box
        x1, x2, y1, y2 = (np.fmin(np.fmax(a, dt(0)), fS) for a in (x1, x2, y1, y2))
        keep &= (x1 < x2 - dt(10)) & (y1 < y2 - dt(10))
        pix = np.stack([x1, y1, x2, y2], 1)
        res = pix / fS
    assert res.dtype == dt
    return res, keep, canvas, pix


def augment_boxes_ref(bank_boxes, bank_labels, offsets, cells, crop, P, k, S, dt=np.float32, M64=None, scale64=None):
    """-> (boxes (T, 4) dt, labels (T,) int64, img (T,) float32, counts (B,) int32) in (image, cell (r, c), source) order.
    dt = float64 takes the matrices and scales from M64 (n_cells, 3, 3) / scale64 (n_cells,) instead of the table's fp32 words."""
    c = parse_cells(cells)
    B, n = len(crop), len(offsets) - 1
    ob, ol, oi, counts = [], [], [], np.zeros(B, np.int32)
    for b in range(B):
        cx, cy = int(crop[b][0]), int(crop[b][1])
        if not (0 <= cx <= k * P - S and 0 <= cy <= k * P - S):
            continue
        for j in range(k * k):
            ci = b * k * k + j
            src = int(c['src'][ci])
            if not 0 <= src < n:
                continue
            lo, hi = int(offsets[src]), int(offsets[src + 1])
            if not (0 <= lo <= hi <= len(bank_boxes)) or hi == lo:
                continue
            M = c['M'][ci] if M64 is None else np.asarray(M64[ci]).reshape(9)
            sc = c['scale'][ci] if scale64 is None else scale64[ci]
            res, keep, _, _ = warp_box(bank_boxes[lo:hi], M, sc, int(c['flags'][ci]), j // k, j % k, P, S, cx, cy, dt)
            ob.append(res[keep])
            ol.append(np.asarray(bank_labels[lo:hi])[keep])
            oi.append(np.full(int(keep.sum()), b, np.float32))
            counts[b] += int(keep.sum())
    if not ob:
        return np.zeros((0, 4), dt), np.zeros((0,), np.int64), np.zeros((0,), np.float32), counts
    return np.concatenate(ob), np.concatenate(ol).astype(np.int64), np.concatenate(oi), counts
