"""CPU restatement of csrc/augment_masks.hip (a helper next to augment_ref.py, not a test): the formulas of include/hdyolo.h, 'instance masks
through the device augmentation', in numpy — fp32 with every operation rounded on its own (numpy never contracts), integers elsewhere.  The
membership of EVERY canvas pixel of a cell is computed (the kernel scans a region it derives from the object's box): a region that is too
small shows as a difference.  What augment_ref.py already restates (the cell table, the corner box and the box pipeline of an object without
a mask) is imported from there."""
import numpy as np

import augment_ref as ref
from augment_ref import F_HFLIP, F_PERSP, F_TRANSPOSE, F_VFLIP

BACKGROUND = 0xFFFF
SIDE = 28
f32 = np.float32


def canvas_owner(inst, src, Minv, flags, P):
    """(P, P) int64 [v][u]: the owner (object index within tile `src`, or BACKGROUND) of every canvas pixel of a cell — the value of the
    instance map at the source pixel nearest to the pixel's source position; BACKGROUND where that is outside the tile, far away or NaN."""
    n, H, W = inst.shape
    own = np.full((P, P), BACKGROUND, np.int64)
    if not 0 <= src < n:
        return own
    v, u = np.meshgrid(np.arange(P), np.arange(P), indexing='ij')
    fu, fv = u.astype(f32), v.astype(f32)
    m = np.asarray(Minv, f32)
    with np.errstate(all='ignore'):
        sx = (m[0] * fu + m[1] * fv) + m[2]
        sy = (m[3] * fu + m[4] * fv) + m[5]
        if flags & F_PERSP:
            sw = (m[6] * fu + m[7] * fv) + m[8]
            sx, sy = sx / sw, sy / sw
        tx, ty = sx * f32(32), sy * f32(32)
        assert tx.dtype == f32
        lim = f32(16777216.0)
        ok = (tx >= -lim) & (tx <= lim) & (ty >= -lim) & (ty <= lim)
    qx = np.rint(np.where(ok, tx, 0)).astype(np.int64)
    qy = np.rint(np.where(ok, ty, 0)).astype(np.int64)
    xn, yn = (qx + 16) >> 5, (qy + 16) >> 5
    ok &= (xn >= 0) & (xn < W) & (yn >= 0) & (yn < H)
    own[ok] = inst[src][yn[ok], xn[ok]]
    return own


def canvas_to_image(u, v, flags, r, c, P, cx, cy):
    """the image position of canvas pixels (u, v) of cell (r, c): hflip, vflip, transpose, the cell's and the crop's offsets"""
    if flags & F_HFLIP:
        u = P - 1 - u
    if flags & F_VFLIP:
        v = P - 1 - v
    if flags & F_TRANSPOSE:
        u, v = v, u
    return u + c * P - cx, v + r * P - cy


def cells_of(bank_offsets, cells, crop, P, k, S, n_boxes):
    """yield (ci, b, r, c, src, lo, count) for every cell that owns candidates, in candidate order"""
    c = ref.parse_cells(cells)
    n = len(bank_offsets) - 1
    for b in range(len(crop)):
        cx, cy = int(crop[b][0]), int(crop[b][1])
        if not (0 <= cx <= k * P - S and 0 <= cy <= k * P - S):
            continue
        for j in range(k * k):
            ci = b * k * k + j
            src = int(c['src'][ci])
            if not 0 <= src < n:
                continue
            lo, hi = int(bank_offsets[src]), int(bank_offsets[src + 1])
            if not (0 <= lo <= hi <= n_boxes) or hi == lo:
                continue
            yield ci, b, j // k, j % k, src, lo, min(hi - lo, 65536)


def mask_extents_ref(inst, has_mask, offsets, n_boxes, cells, crop, P, k, S, pitch):
    """-> (records int32 (n_cells, pitch, 8), written bool (n_cells, pitch)): the record of every candidate, zeros elsewhere"""
    c = ref.parse_cells(cells)
    n_cells = len(cells)
    rec = np.zeros((n_cells, pitch, 8), np.int32)
    written = np.zeros((n_cells, pitch), bool)
    for ci, b, r, cc, src, lo, cnt in cells_of(offsets, cells, crop, P, k, S, n_boxes):
        flags = int(c['flags'][ci])
        own = canvas_owner(inst, src, c['Minv'][ci], flags, P)
        cx, cy = int(crop[b][0]), int(crop[b][1])
        for w in range(min(cnt, pitch)):
            written[ci, w] = True
            if w >= BACKGROUND or not has_mask[lo + w]:
                continue
            vs, us = np.nonzero(own == w)
            if not len(us):
                continue
            ox, oy = canvas_to_image(us, vs, flags, r, cc, P, cx, cy)
            area = int(((ox >= 0) & (ox < S) & (oy >= 0) & (oy < S)).sum())
            rec[ci, w, :6] = (len(us), us.min(), us.max(), vs.min(), vs.max(), area)
    return rec, written


def box_tail(box, nb, thr, scale, flags, r, c, P, S, cx, cy):
    """one source box and its canvas box `nb` through the candidate test at `thr` and everything behind it, fp32 -> (box / S (4,), keep,
    the filter that dropped it: None | 'candidate' | 'crop' | 'final'); the text of augment_ref.warp_box behind its corner box, with the area
    threshold as a parameter"""
    dt = f32
    box, nb = np.asarray(box, dt), np.asarray(nb, dt)
    sc, fP, fS, eps = dt(scale), dt(P), dt(S), dt(1e-16)
    with np.errstate(all='ignore'):
        w1, h1 = box[2] * sc - box[0] * sc, box[3] * sc - box[1] * sc
        w2, h2 = nb[2] - nb[0], nb[3] - nb[1]
        ar = np.fmax(w2 / (h2 + eps), h2 / (w2 + eps))
        cand = bool((w2 > dt(2)) & (h2 > dt(2)) & ((w2 * h2) / (w1 * h1 + eps) > dt(thr)) & (ar < dt(100)))
        x1, y1, x2, y2 = nb
        if flags & F_HFLIP:
            x1, x2, y1, y2 = np.abs(x2 - fP), np.abs(x1 - fP), np.abs(y1), np.abs(y2)
        if flags & F_VFLIP:
            y1, y2, x1, x2 = np.abs(y2 - fP), np.abs(y1 - fP), np.abs(x1), np.abs(x2)
        if flags & F_TRANSPOSE:
            x1, y1, x2, y2 = y1, x1, y2, x2
        ox, oy = dt(c * P) - dt(cx), dt(r * P) - dt(cy)
        x1, x2, y1, y2 = x1 + ox, x2 + ox, y1 + oy, y2 + oy
        in_crop = bool((x1 < x2) & (y1 < y2))
        x1, x2, y1, y2 = (np.fmin(np.fmax(a, dt(0)), fS) for a in (x1, x2, y1, y2))
        final = bool((x1 < x2 - dt(10)) & (y1 < y2 - dt(10)))
        res = np.array([x1, y1, x2, y2], dt) / fS
    assert res.dtype == dt
    why = 'candidate' if not cand else 'crop' if not in_crop else 'final' if not final else None
    return res, why is None, why


def boxes_masks_ref(bank_boxes, bank_labels, has_mask, offsets, cells, crop, P, k, S, rec, pitch, stats=None):
    """-> dict(boxes (T, 4) fp32, labels (T,) int64, img (T,) fp32, counts (B,) int32, ref (T, 2) int32, masked (T,) bool): every kept row, in
    (image, cell (r, c), source) order.  `stats`: a dict that collects why rows were dropped / kept (the tests' non-vacuity counts)."""
    c = ref.parse_cells(cells)
    B = len(crop)
    ob, ol, oi, orf, om, counts = [], [], [], [], [], np.zeros(B, np.int32)
    st = stats if stats is not None else {}
    for key in ('masked_kept', 'unmasked_kept', 'kept_at_001_not_010', 'drop_candidate', 'drop_crop', 'drop_final'):
        st.setdefault(key, 0)
    for ci, b, r, cc, src, lo, cnt in cells_of(offsets, cells, crop, P, k, S, len(bank_boxes)):
        flags, sc = int(c['flags'][ci]), c['scale'][ci]
        cx, cy = int(crop[b][0]), int(crop[b][1])
        plain, plain_keep, _, _ = ref.warp_box(bank_boxes[lo:lo + cnt], c['M'][ci], sc, flags, r, cc, P, S, cx, cy, f32)
        for w in range(cnt):
            masked = w < pitch and w < BACKGROUND and bool(has_mask[lo + w])
            if masked:
                q = rec[ci, w]
                nb = (q[1], q[3], q[2] + 1, q[4] + 1) if q[0] > 0 else (0, 0, 0, 0)
                res, keep, why = box_tail(bank_boxes[lo + w], nb, 0.01, sc, flags, r, cc, P, S, cx, cy)
                if keep and not box_tail(bank_boxes[lo + w], nb, 0.1, sc, flags, r, cc, P, S, cx, cy)[1]:
                    st['kept_at_001_not_010'] += 1
                if not keep:
                    st['drop_' + why] += 1
            else:
                res, keep = plain[w], bool(plain_keep[w])
            if not keep:
                continue
            st['masked_kept' if masked else 'unmasked_kept'] += 1
            ob.append(res)
            ol.append(bank_labels[lo + w])
            oi.append(b)
            orf.append((ci, w))
            om.append(masked)
            counts[b] += 1
    T = len(ob)
    return {'boxes': np.asarray(ob, f32).reshape(T, 4), 'labels': np.asarray(ol, np.int64).reshape(T), 'img': np.asarray(oi, f32).reshape(T),
            'counts': counts, 'ref': np.asarray(orf, np.int32).reshape(T, 2), 'masked': np.asarray(om, bool).reshape(T)}


def image_owner(inst, cells, crop, P, k, S):
    """-> (cell (B, S, S) int64, owner (B, S, S) int64): for every image pixel the cell it shows and the owner of the canvas pixel it shows
    (BACKGROUND for an image whose crop offset is out of range)"""
    c = ref.parse_cells(cells)
    B = len(crop)
    cell = np.full((B, S, S), -1, np.int64)
    owner = np.full((B, S, S), BACKGROUND, np.int64)
    for b in range(B):
        cx, cy = int(crop[b][0]), int(crop[b][1])
        if not (0 <= cx <= k * P - S and 0 <= cy <= k * P - S):
            continue
        Y, X = np.meshgrid(cy + np.arange(S), cx + np.arange(S), indexing='ij')
        cc, rr = X // P, Y // P
        cell[b] = (b * k + rr) * k + cc
        for ci in np.unique(cell[b]):
            sel = cell[b] == ci
            flags = int(c['flags'][ci])
            own = canvas_owner(inst, int(c['src'][ci]), c['Minv'][ci], flags, P)
            u, v = (X - cc * P)[sel], (Y - rr * P)[sel]
            if flags & F_TRANSPOSE:
                u, v = v, u
            if flags & F_VFLIP:
                v = P - 1 - v
            if flags & F_HFLIP:
                u = P - 1 - u
            owner[b][sel] = own[v, u]
    return cell, owner


def image_mask(cell, owner, b, ci, w):
    """the image-space mask (S, S) of object w of cell ci in image b"""
    return (cell[b] == ci) & (owner[b] == w)


def resize_axis(n_src):
    """(x0 (28,), xb (28,), a (28,) fp32) of one axis of the bilinear resize of n_src pixels to 28"""
    j = np.arange(SIDE).astype(f32)
    fx = (j + f32(0.5)) * (f32(n_src) / f32(SIDE)) - f32(0.5)
    x0f = np.floor(fx)
    a = fx - x0f
    x0 = x0f.astype(np.int64)
    a = np.where(x0 < 0, f32(0), a)
    x0 = np.where(x0 < 0, 0, x0)
    a = np.where(x0 >= n_src - 1, f32(0), a)
    x0 = np.where(x0 >= n_src - 1, n_src - 1, x0)
    assert a.dtype == f32
    return x0, np.minimum(x0 + 1, n_src - 1), a


def resize_28(crop_mask):
    """a (h, w) 0/1 mask -> (28, 28) fp32, the header's bilinear formula"""
    m = crop_mask.astype(f32)
    h, w = m.shape
    x0, xb, a = resize_axis(w)
    y0, yb, b = resize_axis(h)
    a, b = a[None, :], b[:, None]
    one = f32(1)
    top = m[y0][:, x0] * (one - a) + m[y0][:, xb] * a
    bot = m[yb][:, x0] * (one - a) + m[yb][:, xb] * a
    out = top * (one - b) + bot * b
    assert out.dtype == f32
    return out


def mask_targets_ref(inst, cells, crop, P, k, S, rec, rows, stats=None):
    """rows: the dict of boxes_masks_ref -> (T, 28, 28) fp32"""
    cell, owner = image_owner(inst, cells, crop, P, k, S)
    T = len(rows['boxes'])
    out = np.zeros((T, SIDE, SIDE), f32)
    st = stats if stats is not None else {}
    for key in ('nonzero_targets', 'zeroed_by_25'):
        st.setdefault(key, 0)
    for t in range(T):
        if not rows['masked'][t]:
            continue
        ci, w = (int(v) for v in rows['ref'][t])
        if rec[ci, w, 5] < 25:
            st['zeroed_by_25'] += 1
            continue
        x1, y1, x2, y2 = (int(min(max(np.rint(v * f32(S)), 0), S)) for v in rows['boxes'][t])
        if x2 - x1 < 1 or y2 - y1 < 1:
            continue
        m = image_mask(cell, owner, int(rows['img'][t]), ci, w)
        out[t] = resize_28(m[y1:y2, x1:x2])
        st['nonzero_targets'] += int(out[t].any())
    return out


def augment_masks_ref(bank, cells, crop, P, k, S, pitch=None, stats=None):
    """the three launches on a TileBank with an instance map -> (records, written, rows dict with 'masks' added)"""
    pitch = max(bank.max_per_tile, 1) if pitch is None else pitch
    rec, written = mask_extents_ref(bank.instances, bank.has_mask, bank.offsets, len(bank.boxes), cells, crop, P, k, S, pitch)
    rows = boxes_masks_ref(bank.boxes, bank.labels, bank.has_mask, bank.offsets, cells, crop, P, k, S, rec, pitch, stats)
    rows['masks'] = mask_targets_ref(bank.instances, cells, crop, P, k, S, rec, rows, stats)
    return rec, written, rows
