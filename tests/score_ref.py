"""numpy restatement of the device AP matching (csrc/score.hip, include/hdyolo.h hdy_ap_match), written from the five steps and not from
the kernel: a dense form (one IoU matrix per image), a cell-binned form for sets too large for a dense matrix, and the chunk-box visit
count.  test_score_host.py ties the dense form to APMeter; test_gpu_score.py ties the device to these.

Per image:
  1. a pair (p, t) with IoU < pair_iou (or NaN) is no pair; a pair whose prediction or truth label is ignored only sets touched[p];
  2. otherwise p keeps the truth of highest IoU, on a tie the lowest truth row;
  3. every truth is claimed by the prediction of highest score among those whose best it is, on a tie the lower prediction row;
  4. p is matched iff it won its claim and the labels agree; hit bit j = best_iou[p] >= iouv[j];
  5. live[p] = not (touched[p] and not matched[p]).
"""
import numpy as np

NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)


def iou_matrix(a, b):
    """utils_general.box_iou in fp32, every operation rounded on its own (numpy never contracts): (n, 4) x (m, 4) -> (n, m)"""
    a, b = np.asarray(a, np.float32).reshape(-1, 4), np.asarray(b, np.float32).reshape(-1, 4)
    with np.errstate(all='ignore'):
        w = np.maximum(np.minimum(a[:, None, 2], b[None, :, 2]) - np.maximum(a[:, None, 0], b[None, :, 0]), np.float32(0))
        h = np.maximum(np.minimum(a[:, None, 3], b[None, :, 3]) - np.maximum(a[:, None, 1], b[None, :, 1]), np.float32(0))
        inter = w * h
        area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
        area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
        return inter / ((area_a[:, None] + area_b[None]) - inter)


def iou_pairs(a, b):
    """the same arithmetic for row-aligned pairs: (n, 4), (n, 4) -> (n,)"""
    with np.errstate(all='ignore'):
        w = np.maximum(np.minimum(a[:, 2], b[:, 2]) - np.maximum(a[:, 0], b[:, 0]), np.float32(0))
        h = np.maximum(np.minimum(a[:, 3], b[:, 3]) - np.maximum(a[:, 1], b[:, 1]), np.float32(0))
        inter = w * h
        return inter / (((a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]) + (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])) - inter)


def desc_key(scores):
    """32-bit key whose ascending unsigned order is descending score order (-0.0 ranks as +0.0)"""
    s = np.asarray(scores, np.float32)
    u = np.where(s == 0, np.uint32(0), s.view(np.uint32)).astype(np.uint32)
    u = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    return ~u


def claim_keys(scores, rows):
    return (desc_key(scores).astype(np.uint64) << np.uint64(32)) | np.asarray(rows).astype(np.uint64)


def _resolve(best, best_iou, touched, scores, pl, tl, prow, n_true, iouv):
    """steps 3-5 from step 2's result"""
    n = len(best)
    has = best >= 0
    key = claim_keys(scores, prow)
    claim = np.full(n_true, NO_KEY, np.uint64)
    np.minimum.at(claim, best[has], key[has])
    matched = np.zeros(n, bool)
    matched[has] = (claim[best[has]] == key[has]) & (pl[has] == tl[best[has]])
    iouv = np.asarray(iouv, np.float32)
    hit = np.zeros(n, np.uint16)
    for j, t in enumerate(iouv):
        hit |= ((matched & (best_iou >= t)).astype(np.uint16) << np.uint16(j)).astype(np.uint16)
    live = ~(touched & ~matched)
    return hit, live.astype(np.uint8), np.where(matched, best, -1).astype(np.int32), np.where(matched, best_iou, np.float32(0)).astype(np.float32)


def match_image(pb, ps, pl, tb, tl, iouv, ignore=(-100, -1), pair_iou=0.5, prow=None, trow=None):
    """dense form, one image: hit (uint16 bits), live (uint8), match (truth index in this image or -1), match_iou (fp32)"""
    pb, tb = np.asarray(pb, np.float32).reshape(-1, 4), np.asarray(tb, np.float32).reshape(-1, 4)
    ps, pl, tl = np.asarray(ps, np.float32), np.asarray(pl, np.int64), np.asarray(tl, np.int64)
    n, m = len(pb), len(tb)
    prow = np.arange(n) if prow is None else np.asarray(prow, np.int64)
    trow = np.arange(m) if trow is None else np.asarray(trow, np.int64)
    ign = list(ignore or ())
    iou = iou_matrix(pb, tb)
    with np.errstate(invalid='ignore'):
        pair = iou >= np.float32(pair_iou)                                  # NaN: no pair
    ignored = np.isin(pl, ign)[:, None] | np.isin(tl, ign)[None] if ign else np.zeros((n, m), bool)
    touched = (pair & ignored).any(1)
    cand = pair & ~ignored
    best = np.full(n, -1, np.int64)
    best_iou = np.zeros(n, np.float32)
    if m:
        masked = np.where(cand, iou, np.float32(-1))
        top = masked.max(1)
        rowkey = np.where(cand & (masked == top[:, None]), trow[None], np.iinfo(np.int64).max)
        arg = rowkey.argmin(1)
        has = cand.any(1)
        best[has] = arg[has]
        best_iou[has] = top[has]
    return _resolve(best, best_iou, touched, ps, pl, tl, prow, m, iouv)


def match_batch(pb, ps, pl, poff, tb, tl, toff, iouv, ignore=(-100, -1), pair_iou=0.5, prow=None, trow=None):
    """dense form over a ragged batch; match holds rows of the concatenated truth array.  Rows outside every span keep the fill values."""
    n = len(ps)
    hit, live, match, miou = np.zeros(n, np.uint16), np.ones(n, np.uint8), np.full(n, -1, np.int32), np.zeros(n, np.float32)
    for i in range(len(poff) - 1):
        p0, p1, t0, t1 = int(poff[i]), int(poff[i + 1]), int(toff[i]), int(toff[i + 1])
        h, l, mt, mi = match_image(pb[p0:p1], ps[p0:p1], pl[p0:p1], tb[t0:t1], tl[t0:t1], iouv, ignore, pair_iou,
                                   None if prow is None else prow[p0:p1], None if trow is None else trow[t0:t1])
        hit[p0:p1], live[p0:p1], miou[p0:p1] = h, l, mi
        match[p0:p1] = np.where(mt >= 0, mt + t0, -1)
    return hit, live, match, miou


def match_binned(pb, ps, pl, tb, tl, iouv, ignore=(-100, -1), pair_iou=0.5, prow=None, trow=None):
    """One image too large for a dense matrix (finite proper boxes only): truths are binned by centre into square cells at least as wide as the
    longest side of any box, so every truth that overlaps a prediction lies in the 3 x 3 cells around the prediction's centre cell; the k-th
    truth of each such cell is met by all predictions at once.  Same steps, same arithmetic, same tie rules as match_image."""
    pb, tb = np.asarray(pb, np.float32).reshape(-1, 4), np.asarray(tb, np.float32).reshape(-1, 4)
    ps, pl, tl = np.asarray(ps, np.float32), np.asarray(pl, np.int64), np.asarray(tl, np.int64)
    n, m = len(pb), len(tb)
    assert np.isfinite(pb).all() and np.isfinite(tb).all()
    prow = np.arange(n) if prow is None else np.asarray(prow, np.int64)
    trow = np.arange(m) if trow is None else np.asarray(trow, np.int64)
    ign = list(ignore or ())
    p_ign, t_ign = (np.isin(pl, ign), np.isin(tl, ign)) if ign else (np.zeros(n, bool), np.zeros(m, bool))
    best, best_iou, best_row = np.full(n, -1, np.int64), np.zeros(n, np.float32), np.zeros(n, np.int64)
    touched = np.zeros(n, bool)
    if n and m:
        both = np.concatenate([pb, tb]).astype(np.float64)
        side = max(float((both[:, 2] - both[:, 0]).max()), float((both[:, 3] - both[:, 1]).max()), 1e-6) * 1.001
        x0, y0 = both[:, [0, 2]].min(), both[:, [1, 3]].min()
        cell = lambda b: (np.floor(((b[:, 0].astype(np.float64) + b[:, 2]) * 0.5 - x0) / side).astype(np.int64) + 1,     # noqa: E731
                          np.floor(((b[:, 1].astype(np.float64) + b[:, 3]) * 0.5 - y0) / side).astype(np.int64) + 1)
        tcx, tcy = cell(tb)
        pcx, pcy = cell(pb)
        gx = int(max(tcx.max(), pcx.max())) + 2
        gy = int(max(tcy.max(), pcy.max())) + 2
        tid = tcy * gx + tcx
        order = np.argsort(tid, kind='stable')
        counts = np.bincount(tid, minlength=gx * gy)
        start = np.concatenate(([0], np.cumsum(counts)))
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                cid = (pcy + dy) * gx + (pcx + dx)
                s, e = start[cid], start[cid + 1]
                for k in range(int((e - s).max()) if len(s) else 0):
                    sel = np.nonzero(s + k < e)[0]
                    t = order[s[sel] + k]
                    iou = iou_pairs(pb[sel], tb[t])
                    with np.errstate(invalid='ignore'):
                        pair = iou >= np.float32(pair_iou)
                    ig = p_ign[sel] | t_ign[t]
                    touched[sel[pair & ig]] = True
                    c = pair & ~ig
                    better = c & ((best[sel] < 0) | (iou > best_iou[sel]) | ((iou == best_iou[sel]) & (trow[t] < best_row[sel])))
                    u = sel[better]
                    best[u], best_iou[u], best_row[u] = t[better], iou[better], trow[t[better]]
    return _resolve(best, best_iou, touched, ps, pl, tl, prow, m, iouv)


def _group_boxes(boxes, size):
    """bounding box (x1, y1, x2, y2) of every run of `size` rows over the rows with finite coordinates, and whether the run holds another"""
    n = len(boxes)
    g = (n + size - 1) // size
    out = np.empty((g, 4), np.float32)
    flag = np.zeros(g, bool)
    for k in range(g):
        b = boxes[k * size:(k + 1) * size]
        ok = np.isfinite(b).all(1)
        flag[k] = not ok.all()
        b = b[ok]
        out[k] = (b[:, 0].min(), b[:, 1].min(), b[:, 2].max(), b[:, 3].max()) if len(b) else (np.inf, np.inf, -np.inf, -np.inf)
    return out, flag


def chunk_visits(pb, poff, tb, toff, block=256, chunk=256):
    """(chunk pairs visited, chunk pairs in total) of the device's pruning rule for this order: per image, a block of `block` prediction rows
    visits a chunk of `chunk` truth rows iff their bounding boxes overlap as closed intervals, or either side holds a non-finite box."""
    pb, tb = np.asarray(pb, np.float32).reshape(-1, 4), np.asarray(tb, np.float32).reshape(-1, 4)
    visited = total = 0
    for i in range(len(poff) - 1):
        bb, bflag = _group_boxes(pb[int(poff[i]):int(poff[i + 1])], block)
        cb, cflag = _group_boxes(tb[int(toff[i]):int(toff[i + 1])], chunk)
        total += len(bb) * len(cb)
        if len(bb) and len(cb):
            overlap = (cb[None, :, 0] <= bb[:, None, 2]) & (bb[:, None, 0] <= cb[None, :, 2]) & \
                      (cb[None, :, 1] <= bb[:, None, 3]) & (bb[:, None, 1] <= cb[None, :, 3])
            visited += int((overlap | bflag[:, None] | cflag[None]).sum())
    return visited, total


class RefMeter:
    """APMeter's surface on top of match_image, for the comparison with APMeter.ap_per_class"""

    def __init__(self, iouv=np.linspace(0.5, 0.95, 10), ignore=(-100, -1)):
        self.iouv, self.ignore = np.asarray(iouv, np.float32), tuple(ignore or ())
        self.scores, self.y_pred, self.y_true, self.hit, self.live = [], [], [], [], []

    def add(self, output, target):
        g = lambda d, k, dt: np.asarray(d[k].detach().cpu().numpy() if hasattr(d[k], 'detach') else d[k]).astype(dt)   # noqa: E731
        ps, pl, tl = g(output, 'scores', np.float32), g(output, 'labels', np.int64), g(target, 'labels', np.int64)
        hit, live, _, _ = match_image(g(output, 'boxes', np.float32), ps, pl, g(target, 'boxes', np.float32), tl, self.iouv, self.ignore)
        for lst, v in zip((self.scores, self.y_pred, self.y_true, self.hit, self.live), (ps, pl, tl, hit, live)):
            lst.append(v)

    def ap_per_class(self):
        from metayolo.models.metrics import ap_curves
        cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)   # noqa: E731
        scores, y_pred, y_true = cat(self.scores, np.float32), cat(self.y_pred, np.int64), cat(self.y_true, np.int64)
        bits, live = cat(self.hit, np.uint16), cat(self.live, bool)
        hit = ((bits[:, None] >> np.arange(len(self.iouv), dtype=np.uint16)[None]) & 1).astype(bool)
        return ap_curves(hit[live], scores[live], y_pred[live], y_true, self.iouv, list(self.ignore))


# ---- seeded inputs shared by the host and the device tests ---------------------------------------------------------------------------
def random_image(rng, n_pred, n_true, nc=3, side=320.0, ignored=0.1, tied_scores=False, dup_truths=False):
    """One image: truths of 10-40 px, predictions that are jittered copies of random truths (some twice, some mislabelled) or hit nothing;
    labels 1..nc with a share of -100 / -1 on both sides; distinct scores unless tied_scores.  dup_truths: every third truth is an exact
    copy of its predecessor (exact IoU ties).  Returns fp32 / int64 numpy arrays (pb, ps, pl, tb, tl)."""
    c = rng.uniform(0, side, (n_true, 2))
    wh = rng.uniform(10, 40, (n_true, 2))
    tb = np.concatenate([c - wh / 2, c + wh / 2], 1).astype(np.float32)
    if dup_truths and n_true > 1:
        k = np.arange(1, n_true, 3)
        tb[k] = tb[k - 1]
    tl = rng.integers(1, nc + 1, n_true).astype(np.int64)
    tl[rng.uniform(0, 1, n_true) < ignored] = rng.choice([-100, -1])
    if n_true:
        src = rng.integers(0, n_true, n_pred)
        near = rng.uniform(0, 1, n_pred) < 0.75
        pc = np.where(near[:, None], (tb[src, :2] + tb[src, 2:]) / 2 + rng.normal(0, 2.0, (n_pred, 2)), rng.uniform(0, side, (n_pred, 2)))
        pwh = np.where(near[:, None], (tb[src, 2:] - tb[src, :2]) * rng.uniform(0.85, 1.15, (n_pred, 2)), rng.uniform(10, 40, (n_pred, 2)))
        exact = near & (rng.uniform(0, 1, n_pred) < 0.1)                   # some predictions sit exactly on their truth: IoU 1
        pl = np.where(near & (rng.uniform(0, 1, n_pred) < 0.8), np.abs(tl[src]) % nc + 1, rng.integers(1, nc + 1, n_pred)).astype(np.int64)
        pl = np.where(near & (tl[src] > 0) & (rng.uniform(0, 1, n_pred) < 0.8), tl[src], pl)
    else:
        pc, pwh = rng.uniform(0, side, (n_pred, 2)), rng.uniform(10, 40, (n_pred, 2))
        exact = np.zeros(n_pred, bool)
        pl = rng.integers(1, nc + 1, n_pred).astype(np.int64)
        src = np.zeros(n_pred, np.int64)
    pb = np.concatenate([pc - pwh / 2, pc + pwh / 2], 1).astype(np.float32)
    if n_true:
        pb[exact] = tb[src[exact]]
    pl[rng.uniform(0, 1, n_pred) < ignored / 2] = -1
    ps = (rng.permutation(n_pred).astype(np.float32) + 1) / np.float32(n_pred + 1)
    if tied_scores and n_pred > 3:
        ps[::3] = ps[0]
    return pb, ps.astype(np.float32), pl, tb, tl


def random_batch(rng, B, max_pred=300, max_true=400, empty=0.15, **kw):
    """B images of 0..max_pred predictions x 0..max_true truths, a share of them empty on either side; concatenated arrays and int32 offsets"""
    parts, n_p, n_t = [], [], []
    for _ in range(B):
        n = 0 if rng.uniform() < empty else int(rng.integers(0, max_pred + 1))
        m = 0 if rng.uniform() < empty else int(rng.integers(0, max_true + 1))
        parts.append(random_image(rng, n, m, **kw))
        n_p.append(n)
        n_t.append(m)
    cat = lambda k: np.concatenate([p[k] for p in parts])   # noqa: E731
    off = lambda c: np.concatenate(([0], np.cumsum(c))).astype(np.int32)   # noqa: E731
    return cat(0).reshape(-1, 4), cat(1), cat(2), off(n_p), cat(3).reshape(-1, 4), cat(4), off(n_t)
