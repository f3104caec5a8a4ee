"""Brute-force restatement of the segmentation summaries (metayolo.models.metrics.segmentation_counts): PQ, per-class PQ, AJI and Dice of two
dense int label maps by plain Python loops over instances.  It shares no code with the torch implementation: pairs come from np.unique on
p * T + t, areas from np.bincount, IoU comparisons go through fractions.Fraction.  A label that is negative or not below the row count is
background; an instance is a row that owns at least one pixel."""
from fractions import Fraction

import numpy as np

INT_KEYS = ('tp', 'fp', 'fn', 'C', 'U', 'inter_sum', 'pred_sum', 'true_sum')


def overlap(pred_map, true_map, n_pred, n_true):
    """(pairs (n, 3) int64 sorted by (p, t), pred_area int32 (n_pred,), true_area int32 (n_true,))"""
    pm, tm = np.asarray(pred_map).astype(np.int64).ravel(), np.asarray(true_map).astype(np.int64).ravel()
    pv, tv = (pm >= 0) & (pm < n_pred), (tm >= 0) & (tm < n_true)
    pa = np.bincount(pm[pv], minlength=n_pred).astype(np.int32)
    ta = np.bincount(tm[tv], minlength=n_true).astype(np.int32)
    both = pv & tv
    keys, cnt = np.unique(pm[both] * max(n_true, 1) + tm[both], return_counts=True)
    pairs = np.stack([keys // max(n_true, 1), keys % max(n_true, 1), cnt], 1).astype(np.int64).reshape(-1, 3)
    return pairs, pa, ta


def counts(pairs, pa, ta, pred_labels=None, true_labels=None, nc=0):
    """the counts of one image (or of one pooled set of rows) as Python numbers; with labels also lists tp_c, fp_c, fn_c, iou_sum_c"""
    pairs = [(int(p), int(t), int(i)) for p, t, i in pairs]
    pa, ta = [int(v) for v in pa], [int(v) for v in ta]
    out = {'inter_sum': sum(i for _, _, i in pairs), 'pred_sum': sum(pa), 'true_sum': sum(ta)}
    # PQ
    matched_p, matched_t, iou_sum = set(), set(), 0.0
    tp_pairs = []
    for p, t, i in pairs:
        if Fraction(i, pa[p] + ta[t] - i) > Fraction(1, 2):
            assert p not in matched_p and t not in matched_t
            matched_p.add(p)
            matched_t.add(t)
            tp_pairs.append((p, t, i))
            iou_sum += i / (pa[p] + ta[t] - i)
    out['tp'] = len(tp_pairs)
    out['fp'] = sum(1 for p in range(len(pa)) if pa[p] > 0 and p not in matched_p)
    out['fn'] = sum(1 for t in range(len(ta)) if ta[t] > 0 and t not in matched_t)
    out['iou_sum'] = iou_sum
    # AJI
    C = U = 0
    used = set()
    for t in range(len(ta)):
        best = None
        for p, tt, i in pairs:
            if tt != t:
                continue
            iou = Fraction(i, pa[p] + ta[t] - i)
            if best is None or iou > best[0] or (iou == best[0] and p < best[1]):
                best = (iou, p, i)
        if best is None:
            U += ta[t]
        else:
            C += best[2]
            U += pa[best[1]] + ta[t] - best[2]
            used.add(best[1])
    for p in range(len(pa)):
        if p not in used:
            U += pa[p]
    out['C'], out['U'] = C, U
    if pred_labels is not None:
        pl, tl = [int(v) for v in pred_labels], [int(v) for v in true_labels]
        out['tp_c'], out['fp_c'], out['fn_c'], out['iou_sum_c'] = [], [], [], []
        for c in range(1, nc + 1):
            mine = [(p, t, i) for p, t, i in tp_pairs if pl[p] == c and tl[t] == c]
            out['tp_c'].append(len(mine))
            out['fp_c'].append(sum(1 for p in range(len(pa)) if pa[p] > 0 and pl[p] == c) - len(mine))
            out['fn_c'].append(sum(1 for t in range(len(ta)) if ta[t] > 0 and tl[t] == c) - len(mine))
            out['iou_sum_c'].append(sum(i / (pa[p] + ta[t] - i) for p, t, i in mine))
    return out


def pool(parts):
    """the sum of several images' counts"""
    out = {}
    for c in parts:
        for k, v in c.items():
            if isinstance(v, list):
                out[k] = [a + b for a, b in zip(out[k], v)] if k in out else list(v)
            else:
                out[k] = out.get(k, 0) + v
    return out


def ratios(c):
    div = lambda a, b: a / b if b else 0.0   # noqa: E731
    dq = div(c['tp'], c['tp'] + c['fp'] / 2 + c['fn'] / 2)
    sq = div(c['iou_sum'], c['tp'])
    out = {'pq': dq * sq, 'sq': sq, 'dq': dq, 'aji': div(c['C'], c['U']), 'dice': div(2 * c['inter_sum'], c['pred_sum'] + c['true_sum'])}
    if 'tp_c' in c:
        per = []
        for tp, fp, fn, s in zip(c['tp_c'], c['fp_c'], c['fn_c'], c['iou_sum_c']):
            if tp + fp + fn > 0:
                per.append(div(tp, tp + fp / 2 + fn / 2) * div(s, tp))
        out['mpq'] = sum(per) / len(per) if per else 0.0
    return out


def random_map(rng, shape, n, extra_rows=0):
    """n instances, random rectangles and discs painted in random order so that they fragment and bury each other; `extra_rows` more rows
    are named in the areas but never painted.  -> (int32 map with -1 background, row count)"""
    H, W = shape
    m = np.full(shape, -1, np.int32)
    yy, xx = np.mgrid[0:H, 0:W]
    for r in rng.permutation(n):
        cy, cx = rng.uniform(0, H), rng.uniform(0, W)
        if rng.random() < 0.5:
            h, w = rng.uniform(2, H / 3), rng.uniform(2, W / 3)
            sel = (abs(yy - cy) <= h / 2) & (abs(xx - cx) <= w / 2)
        else:
            rad = rng.uniform(1.5, min(H, W) / 5)
            sel = (yy - cy) ** 2 + (xx - cx) ** 2 <= rad ** 2
        m[sel] = r
    return m, n + extra_rows
