"""numpy restatement of the device mask scoring (csrc/mask_score.hip, include/hdyolo.h "mask scoring"), written from the stated arithmetic and
not from the kernels: dense contingency counts of two label maps, the IoU from integer counts, and the five matching rules of
tests/score_ref.py on that IoU.  test_mask_score_host.py ties it to the host APMeter and the golden; test_gpu_mask_score.py ties the device to it.

  inter[p, t] = entries where the prediction map holds p and the truth map holds t (labels outside [0, n) after the segment base: background)
  union = area_p + area_t - inter (int64);  iou = float32(inter) / float32(union);  a pair needs inter > 0
  rules 1-5: tests/score_ref.py, for one set of rows (rows of different images never share an entry, hence never a pair).
"""
import numpy as np

import score_ref

f32 = np.float32


def global_rows(label_map, n, base=None):
    """map entries as rows of the concatenated array, -1 = background; base (n_seg,) is added to the non-negative labels of each segment (the
    map's first dimension)"""
    m = np.asarray(label_map).astype(np.int64)
    if base is not None:
        b = np.asarray(base, np.int64).reshape((-1,) + (1,) * (m.ndim - 1))
        m = np.where(m >= 0, m + b, -1)
    return np.where((m >= 0) & (m < n), m, -1).reshape(-1)


def overlap(pred_map, true_map, n_pred, n_true, pred_base=None, true_base=None):
    """(pairs (n, 3) int64 sorted by (p, t) with inter > 0, pred_area int32, true_area int32)"""
    p, t = global_rows(pred_map, n_pred, pred_base), global_rows(true_map, n_true, true_base)
    assert p.shape == t.shape
    pa, ta = np.zeros(n_pred, np.int64), np.zeros(n_true, np.int64)
    np.add.at(pa, p[p >= 0], 1)
    np.add.at(ta, t[t >= 0], 1)
    inter = np.zeros((n_pred, n_true), np.int64)
    both = (p >= 0) & (t >= 0)
    np.add.at(inter, (p[both], t[both]), 1)
    pi, ti = np.nonzero(inter)                                       # row-major: sorted by (p, t)
    return np.stack([pi, ti, inter[pi, ti]], 1).astype(np.int64).reshape(-1, 3), pa.astype(np.int32), ta.astype(np.int32)


def pair_ious(pairs, pred_area, true_area):
    """the stated IoU of every pair: one fp32 division of the two conversions"""
    inter = pairs[:, 2].astype(np.int64)
    union = pred_area.astype(np.int64)[pairs[:, 0]] + true_area.astype(np.int64)[pairs[:, 1]] - inter
    return inter.astype(f32) / union.astype(f32)


def iou_matrix(pairs, pred_area, true_area):
    """dense (n_pred, n_true) fp32: the stated IoU where a pair exists, 0 elsewhere"""
    iou = np.zeros((len(pred_area), len(true_area)), f32)
    iou[pairs[:, 0], pairs[:, 1]] = pair_ious(pairs, pred_area, true_area)
    return iou


def match(pairs, pred_area, true_area, ps, pl, tl, iouv, ignore=(-100, -1), pair_iou=0.5, prow=None, trow=None):
    """rules 1-5 on the mask IoU: hit (uint16 bits), live (uint8), match (truth row or -1), match_iou (fp32), one per prediction"""
    ps, pl, tl = np.asarray(ps, f32), np.asarray(pl, np.int64), np.asarray(tl, np.int64)
    n, m = len(ps), len(tl)
    prow = np.arange(n) if prow is None else np.asarray(prow, np.int64)
    trow = np.arange(m) if trow is None else np.asarray(trow, np.int64)
    ign = list(ignore or ())
    iou = iou_matrix(pairs, pred_area, true_area)
    pair = iou >= f32(pair_iou)                                       # (no pair without a shared entry: iou 0 < pair_iou)
    ignored = np.isin(pl, ign)[:, None] | np.isin(tl, ign)[None] if ign else np.zeros((n, m), bool)
    touched = (pair & ignored).any(1)
    cand = pair & ~ignored
    best = np.full(n, -1, np.int64)
    best_iou = np.zeros(n, f32)
    if m and n:
        masked = np.where(cand, iou, f32(-1))
        top = masked.max(1)
        rowkey = np.where(cand & (masked == top[:, None]), trow[None], np.iinfo(np.int64).max)
        arg = rowkey.argmin(1)
        has = cand.any(1)
        best[has] = arg[has]
        best_iou[has] = top[has]
    return score_ref._resolve(best, best_iou, touched, ps, pl, tl, prow, m, iouv)


def dense_masks(label_map, n):
    """(n, H, W) fp32 0 / 1 masks of rows 0 .. n - 1 of one label map"""
    m = np.asarray(label_map).astype(np.int64)
    return (m[None] == np.arange(n).reshape(-1, 1, 1)).astype(f32)


class RefMeter:
    """APMeter's surface on top of overlap + match, fed label maps, for the comparison with APMeter(iou_type='masks')"""

    def __init__(self, iouv=np.linspace(0.5, 0.95, 10), ignore=(-100, -1)):
        self.iouv, self.ignore = np.asarray(iouv, f32), tuple(ignore or ())
        self.scores, self.y_pred, self.y_true, self.hit, self.live = [], [], [], [], []

    def add(self, pred_map, ps, pl, true_map, tl):
        ps, pl, tl = np.asarray(ps, f32), np.asarray(pl, np.int64), np.asarray(tl, np.int64)
        pairs, pa, ta = overlap(pred_map, true_map, len(ps), len(tl))
        hit, live, _, _ = match(pairs, pa, ta, ps, pl, tl, self.iouv, self.ignore)
        for lst, v in zip((self.scores, self.y_pred, self.y_true, self.hit, self.live), (ps, pl, tl, hit, live)):
            lst.append(v)

    ap_per_class = score_ref.RefMeter.ap_per_class


# ---- seeded label maps shared by the golden script, the host and the device tests ---------------------------------------------------------
def draw_ellipses(shape, specs, n_max=None):
    """A label map of disjoint instances: spec k = (cy, cx, ry, rx) is drawn where the canvas is still background, so earlier rows own overlaps.
    Returns the int32 map (-1 background)."""
    H, W = shape
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.full((H, W), -1, np.int32)
    for k, (cy, cx, ry, rx) in enumerate(specs):
        inside = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
        out[inside & (out < 0)] = k
    return out


def ellipse_pair(rng, shape, n_true, r=(3.5, 6.5), keep=0.85, extra=0.15):
    """One image: truth and prediction label maps.  Predictions are the truths moved by -1 .. 2 pixels and grown / shrunk by up to a pixel
    (most pairs pass IoU 0.5), some dropped, some added, in shuffled row order.  Returns (pred_map, true_map, n_pred, source) with
    source[p] = the truth a prediction was made from, or -1."""
    H, W = shape
    tspec = [(rng.uniform(2, H - 2), rng.uniform(2, W - 2), rng.uniform(*r), rng.uniform(*r)) for _ in range(n_true)]
    pspec, source = [], []
    for k, (cy, cx, ry, rx) in enumerate(tspec):
        if rng.uniform() < keep:
            pspec.append((cy + rng.integers(-1, 3), cx + rng.integers(-1, 3), max(1.2, ry + rng.uniform(-1.0, 1.0)), max(1.2, rx + rng.uniform(-1.0, 1.0))))
            source.append(k)
    for _ in range(int(round(extra * n_true))):
        pspec.append((rng.uniform(2, H - 2), rng.uniform(2, W - 2), rng.uniform(*r), rng.uniform(*r)))
        source.append(-1)
    order = rng.permutation(len(pspec))
    pspec, source = [pspec[i] for i in order], np.asarray([source[i] for i in order], np.int64)
    return draw_ellipses(shape, pspec), draw_ellipses(shape, tspec), len(pspec), source


def labels_and_scores(rng, n_pred, n_true, source, nc=3, wrong=0.15, ignored=0.1):
    """truth labels 1 .. nc with a share of -1 (ignored); prediction labels follow their source truth (a share disagrees, a few are ignored
    themselves); distinct scores"""
    tl = rng.integers(1, nc + 1, n_true).astype(np.int64)
    tl[rng.uniform(0, 1, n_true) < ignored] = -1
    pl = rng.integers(1, nc + 1, n_pred).astype(np.int64)
    follow = (source >= 0) & (rng.uniform(0, 1, n_pred) >= wrong)
    pl[follow] = np.where(tl[source[follow]] > 0, tl[source[follow]], pl[follow])
    pl[rng.uniform(0, 1, n_pred) < ignored / 3] = -1
    ps = ((rng.permutation(n_pred) + 1 + rng.uniform(0, 0.5, n_pred)) / (n_pred + 1)).astype(f32)      # (jittered: distinct across images too)
    return ps, pl, tl


def paste_inputs(label_map, n, M=28):
    """(masks (n, 1, M, M) fp32 0 / 1, boxes (n, 4) fp32) that the mask paste (padding 1, threshold 0.5) turns back into `label_map` exactly,
    for disjoint instances no wider or taller than M: every box expands (by P / M about its centre, P = M + 2) to an integer box of exactly
    P x P pixels, so the resize is the identity and mask entry (my, mx) lands on canvas pixel (Y0 + 1 + my, X0 + 1 + mx) with value 0 or 1.
    The expanded corners sit a quarter pixel inside their integer cell on the side that truncation toward zero keeps."""
    lm = np.asarray(label_map).astype(np.int64)
    H, W = lm.shape
    P = M + 2
    masks, boxes = np.zeros((n, 1, M, M), f32), np.zeros((n, 4), f32)
    for r in range(n):
        ys, xs = np.nonzero(lm == r)
        y0, x0 = (int(ys.min()), int(xs.min())) if len(ys) else (0, 0)
        if len(ys):
            assert ys.max() - y0 < M and xs.max() - x0 < M, 'instance larger than the mask'
            masks[r, 0, ys - y0, xs - x0] = 1
        corner = lambda v: v + 0.25 if v >= 0 else v - 0.25   # noqa: E731      (int() truncates toward zero)
        e = [corner(x0 - 1), corner(y0 - 1), corner(x0 - 1 + P - 1), corner(y0 - 1 + P - 1)]
        cx, cy, hx, hy = (e[0] + e[2]) / 2, (e[1] + e[3]) / 2, (e[2] - e[0]) / 2 * M / P, (e[3] - e[1]) / 2 * M / P
        boxes[r] = (cx - hx, cy - hy, cx + hx, cy + hy)
    return masks, boxes
