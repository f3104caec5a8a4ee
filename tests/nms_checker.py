"""TEST INFRASTRUCTURE ONLY: checks that an index list IS the greedy NMS of a box set, without running a greedy pass.

Greedy NMS is the unique solution of:  box i is kept  <=>  no kept box of higher rank has IoU(i, j) > thr  (rank = descending score,
ties by lower row).  Uniqueness follows by induction over the rank, so verifying the equivalence for every box, plus the order of `keep`,
proves equality with the sequential pass.  The pairs that can have a positive IoU are found by a spatial join in numpy (bin by centre, cell
>= the longest side, 3 x 3 window), so the check costs O(M x neighbours) and serves sizes the O(M x kept) oracle cannot.  IoU in fp32 in
the oracle's operation order (oracle/nms_ref.c)."""
import numpy as np


def iou_gt(a, b, thr):
    f = np.float32
    xx1 = np.maximum(a[:, 0], b[:, 0]); yy1 = np.maximum(a[:, 1], b[:, 1])
    xx2 = np.minimum(a[:, 2], b[:, 2]); yy2 = np.minimum(a[:, 3], b[:, 3])
    w = np.maximum(f(0), xx2 - xx1); h = np.maximum(f(0), yy2 - yy1)
    inter = w * h
    aa = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]); ab = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    with np.errstate(divide='ignore', invalid='ignore'):
        return inter / ((aa + ab) - inter) > f(thr)


def candidate_pairs(boxes):
    """All (i, j), i != j, of PROPER boxes whose extents can intersect.  Cell = longest side (so centres of intersecting boxes are less
    than one cell apart per axis) x 1.001 against the rounding of the centre."""
    n = len(boxes)
    proper = (boxes[:, 2] > boxes[:, 0]) & (boxes[:, 3] > boxes[:, 1])
    idx = np.nonzero(proper)[0]
    if len(idx) < 2:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    b = boxes[idx].astype(np.float64)
    cell = float(max((b[:, 2] - b[:, 0]).max(), (b[:, 3] - b[:, 1]).max())) * 1.001
    c = (b[:, :2] + b[:, 2:]) / 2
    g = np.floor(c / cell).astype(np.int64)
    g -= g.min(0)
    W = int(g[:, 0].max()) + 3
    key = (g[:, 1] + 1) * W + g[:, 0] + 1
    o = np.argsort(key, kind='stable')
    ks = key[o]
    out_i, out_j = [], []
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            nk = key + dy * W + dx
            lo = np.searchsorted(ks, nk, 'left'); hi = np.searchsorted(ks, nk, 'right')
            cnt = hi - lo
            i = np.repeat(np.arange(len(b)), cnt)
            off = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
            out_i.append(i)
            out_j.append(o[np.repeat(lo, cnt) + off])
    i = np.concatenate(out_i); j = np.concatenate(out_j)
    m = i != j
    return idx[i[m]], idx[j[m]]


def is_greedy_nms(boxes, scores, thr, keep):
    boxes = np.ascontiguousarray(boxes, dtype=np.float32)
    scores = np.ascontiguousarray(scores, dtype=np.float32)
    keep = np.asarray(keep, dtype=np.int64)
    n = len(boxes)
    if len(keep) and (keep.min() < 0 or keep.max() >= n or len(np.unique(keep)) != len(keep)):
        return False, 'keep holds an index outside the set or twice'
    rank = np.empty(n, np.int64)
    rank[np.argsort(-scores, kind='stable')] = np.arange(n)
    if not (np.diff(rank[keep]) > 0).all():
        return False, 'keep is not in rank order'
    kept = np.zeros(n, bool)
    kept[keep] = True
    i, j = candidate_pairs(boxes)
    hit = iou_gt(boxes[j], boxes[i], thr) & (rank[j] < rank[i]) & kept[j]          # j: a kept box of higher rank over i
    has = np.zeros(n, bool)
    has[i[hit]] = True
    bad = np.nonzero(has == kept)[0]                                             # kept <=> no such j
    if len(bad):
        r = int(bad[0])
        return False, f'{len(bad)} boxes violate the rule, first row {r}: kept={bool(kept[r])}, higher-ranked kept overlap={bool(has[r])}'
    return True, ''


def assert_is_greedy_nms(boxes, scores, thr, keep):
    ok, why = is_greedy_nms(boxes, scores, thr, keep)
    assert ok, why
