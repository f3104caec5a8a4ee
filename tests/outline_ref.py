"""Restatement of include/hdyolo_outline.h (csrc/outline.hip) built differently from the kernels: where the kernel walks crack by crack, this
takes the label's first 4-connected component from scipy.ndimage.label, fills its holes (the 8-connected background parts of the padded box
that do not reach the frame), collects the SET of directed boundary cracks of the filled component, links each crack to its successor at its
end corner and reads the cycle off from the start crack.  The hull is Andrew's monotone chain over ALL corners of the label's pixels sorted by
(x, y) in Python integers (the kernel sorts by y and keeps two corners per lattice row), the maximum Feret diameter a brute force over corner
pairs in int64, perimeter and minimum Feret diameter float64 from the exact hull.  `rasterise` is a deliberately slow second form of the
outline: the polygon filled by the even-odd rule at pixel centres.  `shape_row` restates hd_yolo_amd/outline.py's shape_table one row at a time."""
import math

import numpy as np
from scipy import ndimage

MAX_SIDE = 1024
FOUR = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])
EIGHT = np.ones((3, 3), dtype=int)
STEP = ((1, 0), (0, 1), (-1, 0), (0, -1))        # directions 0: +x, 1: +y (down), 2: -x, 3: -y


def clamped_box(ext, h, w):
    """(bx0, by0, bw, bh, flag) of an extent row {min j, min i, max j, max i}"""
    ex0, ey0, ex1, ey1 = (int(v) for v in ext)
    x0, y0, x1, y1 = max(ex0, 0), max(ey0, 0), min(ex1, w - 1), min(ey1, h - 1)
    if x1 < x0 or y1 < y0:
        return 0, 0, 0, 0, 1
    bw, bh = x1 - x0 + 1, y1 - y0 + 1
    return x0, y0, bw, bh, 2 if bw > MAX_SIDE or bh > MAX_SIDE else 0


def filled_component(lm, r, i0, j0):
    """(K, filled, (top, left)): the 4-connected component of {lm == r} through (i0, j0) and the same with its holes, as boolean arrays over
    the component's bounding box grown by one pixel on every side, whose corner in the map is (top, left)"""
    ii, jj = np.nonzero(lm == r)
    t, l = int(ii.min()), int(jj.min())                                   # scipy labels the label's bounding box, not the whole map
    own = np.zeros((int(ii.max()) - t + 1, int(jj.max()) - l + 1), dtype=bool)
    own[ii - t, jj - l] = True
    lab, _ = ndimage.label(own, structure=FOUR)
    ii, jj = np.nonzero(lab == lab[i0 - t, j0 - l])
    ii, jj = ii + t, jj + l
    top, left = int(ii.min()) - 1, int(jj.min()) - 1
    pad = np.zeros((int(ii.max()) - top + 2, int(jj.max()) - left + 2), dtype=bool)
    pad[ii - top, jj - left] = True
    back, _ = ndimage.label(~pad, structure=EIGHT)
    holes = ~pad & (back != back[0, 0])                                    # the frame is background and one 8-connected part
    return pad, pad | holes, (top, left)


def boundary_cracks(F, top, left):
    """the set of directed cracks ((x, y), d) of a boolean array with the foreground on the right of every crack, in map coordinates"""
    cracks = set()
    H, W = F.shape
    for i, j in zip(*np.nonzero(F)):
        i, j = int(i), int(j)
        x, y = j + left, i + top
        if i == 0 or not F[i - 1, j]:
            cracks.add(((x, y), 0))                                       # the top edge, heading +x
        if j == W - 1 or not F[i, j + 1]:
            cracks.add(((x + 1, y), 1))                                   # the right edge, heading +y
        if i == H - 1 or not F[i + 1, j]:
            cracks.add(((x + 1, y + 1), 2))                               # the bottom edge, heading -x
        if j == 0 or not F[i, j - 1]:
            cracks.add(((x, y + 1), 3))                                   # the left edge, heading -y
    return cracks


def outline(lm, r, ext):
    """(verts int32 (V, 2), twice the enclosed area, cracks L, flag) of label r; a flagged label has no vertices and zeros"""
    lm = np.asarray(lm)
    h, w = lm.shape
    none = (np.zeros((0, 2), dtype=np.int32), 0, 0)
    x0, y0, bw, bh, flag = clamped_box(ext, h, w)
    if flag:
        return none + (flag,)
    hits = np.nonzero(lm[y0, x0:x0 + bw] == r)[0]
    if len(hits) == 0:
        return none + (4,)
    i0, j0 = y0, x0 + int(hits[0])
    if (i0 > 0 and lm[i0 - 1, j0] == r) or (j0 > 0 and lm[i0, j0 - 1] == r):
        return none + (4,)
    _, F, (top, left) = filled_component(lm, r, i0, j0)
    cracks = boundary_cracks(F, top, left)
    start = ((j0, i0), 0)
    if start not in cracks:                                               # the pixel above s lies in a hole of K
        return none + (4,)
    leaving = {}
    for c, d in cracks:
        leaving.setdefault(c, []).append(d)
    verts, L, (c, d) = [(j0, i0)], 0, start
    while True:
        c = (c[0] + STEP[d][0], c[1] + STEP[d][1])
        L += 1
        out = leaving[c]
        # one crack leaves an ordinary corner; two leave a corner where the component touches itself diagonally, and the walk takes the one
        # that stays with its own pixel: the turn to the right
        nd = out[0] if len(out) == 1 else (d + 1) % 4
        assert nd in out and nd != (d + 2) % 4
        if (c, nd) == start:
            break
        if nd != d:
            verts.append(c)
        d = nd
    if L > bw * (bh + 1) + bh * (bw + 1):
        return none + (4,)
    v = np.asarray(verts, dtype=np.int64)
    nxt = np.roll(v, -1, axis=0)
    area2 = int((v[:, 0] * nxt[:, 1] - nxt[:, 0] * v[:, 1]).sum())
    return v.astype(np.int32), area2, L, 0


def outlines(lm, R, extent):
    """(offsets int64 (R + 1,), verts int32 (total, 2), counts int64 (R, 4)) as ops.label_outline returns them"""
    rows, counts = [], np.zeros((R, 4), dtype=np.int64)
    for r in range(R):
        v, area2, L, flag = outline(lm, r, extent[r])
        rows.append(v)
        counts[r] = (len(v), area2, L, flag)
    offsets = np.zeros((R + 1,), dtype=np.int64)
    offsets[1:] = np.cumsum(counts[:, 0])
    verts = np.concatenate(rows, 0).astype(np.int32) if rows else np.zeros((0, 2), dtype=np.int32)
    return offsets, verts.reshape(-1, 2), counts


def rasterise(verts, h, w):
    """the (h, w) boolean image of a rectilinear polygon by the even-odd rule at pixel centres: pixel (i, j) is inside when an odd number of
    vertical edges crosses the ray from its centre to the left"""
    img = np.zeros((h, w), dtype=bool)
    v = [(int(x), int(y)) for x, y in verts]
    for (ax, ay), (bx, by) in zip(v, v[1:] + v[:1]):
        if ax == bx and ay != by:
            for i in range(min(ay, by), max(ay, by)):
                for j in range(ax, w):
                    img[i, j] = not img[i, j]
    return img


def _cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def hull_points(points):
    """Andrew's monotone chain over a set of integer points, collinear points dropped; the vertices in some cyclic order"""
    pts = sorted(set(points))
    if len(pts) < 3:
        return pts
    lower, upper = [], []
    for p in pts:
        while len(lower) >= 2 and _cross(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    for p in reversed(pts):
        while len(upper) >= 2 and _cross(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    return lower[:-1] + upper[:-1]


BRUTE = 400        # corners up to which the maximum Feret diameter is a brute force over ALL corner pairs


def hull(lm, r, ext):
    """((H, twice the hull area, squared maximum Feret diameter, flag), (perimeter, minimum Feret diameter)) of label r"""
    lm = np.asarray(lm)
    h, w = lm.shape
    x0, y0, bw, bh, flag = clamped_box(ext, h, w)
    if not flag and not (lm[y0, x0:x0 + bw] == r).any():
        flag = 4
    if flag:
        return (0, 0, 0, flag), (0.0, 0.0)
    ii, jj = np.nonzero(lm[y0:y0 + bh, x0:x0 + bw] == r)
    ii, jj = ii + y0, jj + x0
    corners = np.unique(np.concatenate([np.stack([jj + a, ii + b], 1) for a in (0, 1) for b in (0, 1)]), axis=0).astype(np.int64)
    hv = hull_points([(int(x), int(y)) for x, y in corners])
    H = len(hv)
    nxt = hv[1:] + hv[:1]
    area2 = abs(sum(a[0] * b[1] - b[0] * a[1] for a, b in zip(hv, nxt)))
    far = corners if len(corners) <= BRUTE else np.asarray(hv, dtype=np.int64)      # a larger set: the farthest pair is a pair of hull corners
    dx, dy = far[:, None, 0] - far[None, :, 0], far[:, None, 1] - far[None, :, 1]
    fmax2 = int((dx * dx + dy * dy).max())
    perimeter = float(sum(math.sqrt((b[0] - a[0]) ** 2 + (b[1] - a[1]) ** 2) for a, b in zip(hv, nxt)))
    widths = []
    for a, b in zip(hv, nxt):
        reach = max(abs(_cross(a, b, p)) for p in hv)
        widths.append(reach / math.sqrt((b[0] - a[0]) ** 2 + (b[1] - a[1]) ** 2))
    return (H, area2, fmax2, 0), (perimeter, min(widths))


def hulls(lm, R, extent):
    """(hull_i int64 (R, 4), hull_f float64 (R, 2)) as ops.label_hull returns them"""
    hull_i, hull_f = np.zeros((R, 4), dtype=np.int64), np.zeros((R, 2), dtype=np.float64)
    for r in range(R):
        hull_i[r], hull_f[r] = hull(lm, r, extent[r])
    return hull_i, hull_f


def shape_row(n, edges, count, hi, hf):
    """one row of hd_yolo_amd/outline.py's shape_table in Python numbers"""
    V, area2, L, flag = (int(v) for v in count)
    H, hull2, fmax2, hflag = (int(v) for v in hi)
    ok = n > 0 and flag == 0 and hflag == 0
    nan = float('nan')
    row = {'outline_vertices': V, 'outline_edges': L, 'enclosed_area': area2 // 2, 'simple': ok and area2 // 2 == n and L == edges}
    row['convex_area'] = hull2 / 2 if ok else nan
    row['solidity'] = 2 * n / hull2 if ok else nan
    row['convex_perimeter'] = float(hf[0]) if ok else nan
    row['convexity'] = float(hf[0]) / L if ok else nan
    row['feret_max'] = math.sqrt(fmax2) if ok else nan
    row['feret_min'] = float(hf[1]) if ok else nan
    row['feret_ratio'] = float(hf[1]) / math.sqrt(fmax2) if ok else nan
    return row


def shape(text, label=0, background=-1):
    """an int32 map from rows of '#' (the label) and '.' (background)"""
    rows = text.split()
    return np.array([[label if ch == '#' else background for ch in row] for row in rows], dtype=np.int32)


S2 = math.sqrt(2.0)
# name -> (map of label 0, outline vertices, twice the enclosed area, cracks, n, simple, (H, twice the hull area, squared Feret max), (hull
# perimeter, Feret min)), every answer derived by hand from the statement in include/hdyolo_outline.h
HAND = {
    'pixel': (shape('#'), [(0, 0), (1, 0), (1, 1), (0, 1)], 2, 4, 1, True, (4, 2, 2), (4.0, 1.0)),
    'row': (shape('#####'), [(0, 0), (5, 0), (5, 1), (0, 1)], 10, 12, 5, True, (4, 10, 26), (12.0, 1.0)),
    'L': (shape('#. #. ##'), [(0, 0), (1, 0), (1, 2), (2, 2), (2, 3), (0, 3)], 8, 10, 4, True, (5, 10, 13), (7.0 + math.sqrt(5.0), 2.0)),
    'U': (shape('#.# ###'), [(0, 0), (1, 0), (1, 1), (2, 1), (2, 0), (3, 0), (3, 2), (0, 2)], 10, 12, 5, True, (4, 12, 13), (10.0, 2.0)),
    'plus': (shape('.#. ### .#.'), [(1, 0), (2, 0), (2, 1), (3, 1), (3, 2), (2, 2), (2, 3), (1, 3), (1, 2), (0, 2), (0, 1), (1, 1)], 10, 12, 5,
             True, (8, 14, 10), (4.0 + 4.0 * S2, 2.0 * S2)),
    # the outline of the outer square: the hole counts as enclosed
    'ring': (shape('### #.# ###'), [(0, 0), (3, 0), (3, 3), (0, 3)], 18, 12, 8, False, (4, 18, 18), (12.0, 3.0)),
    # the first pixel only (the second hangs on it by a corner); the hull takes both
    'diagonal': (shape('#. .#'), [(0, 0), (1, 0), (1, 1), (0, 1)], 2, 4, 2, False, (6, 6, 8), (4.0 + 2.0 * S2, S2)),
    # the would-be hole reaches the outside through the missing corner: the walk goes in and out through corner (1, 1), a vertex twice
    'leak': (shape('.## #.# ###'), [(1, 0), (3, 0), (3, 3), (0, 3), (0, 1), (1, 1), (1, 2), (2, 2), (2, 1), (1, 1)], 14, 16, 7, True,
             (5, 17, 18), (10.0 + S2, 3.0)),
    'full': (shape('#### #### ####'), [(0, 0), (4, 0), (4, 3), (0, 3)], 24, 14, 12, True, (4, 24, 25), (14.0, 3.0)),
}
