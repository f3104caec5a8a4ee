"""Detection metrics for the validation entry point (reference: metayolo/models/metrics.py:19-84 ap_per_class,
:86-110 compute_ap, :251-408 APMeter).  APMeter is host-side numpy and keeps the reference's matching rules and stats dictionary
(pinned by tests/golden/apmeter.npz); DeviceAPMeter does the same matching on the device (csrc/score.hip) for batches and whole
slides, and shares the curve arithmetic (ap_curves).  Mask IoU: get_mask_ious defines the name the reference's APMeter.add calls without
defining it (metrics.py:275; the function is utils_nucls.py:480-489), for the host meter's iou_type='masks'; on the device
DeviceAPMeter.add_batch_masks scores label maps (csrc/mask_score.hip).  segmentation_counts / segmentation_ratios form PQ, AJI and Dice from the
same overlap pairs (torch tensor ops, any device; no reference counterpart: the reference's validation stops at pasting the masks)."""
import numpy as np
import torch

from .utils_general import box_iou


def compute_ap(recall, precision):
    """Area under the precision envelope, 101-point interpolation (COCO)."""
    mrec = np.concatenate(([0.0], recall, [1.0]))
    mpre = np.concatenate(([1.0], precision, [0.0]))
    mpre = np.flip(np.maximum.accumulate(np.flip(mpre)))
    x = np.linspace(0, 1, 101)
    y = np.interp(x, mrec, mpre)
    return float(np.sum((y[1:] + y[:-1]) * np.diff(x)) / 2.0), mpre, mrec     # trapezoid rule


def ap_per_class(tp, conf, pred_cls, target_cls, eps=1e-16):
    """tp (n_pred, n_iou) bool, conf / pred_cls (n_pred,), target_cls (n_true,) -> p, r, ap (n_cls, n_iou), f1, classes."""
    order = np.argsort(-conf)
    tp, conf, pred_cls = tp[order], conf[order], pred_cls[order]
    classes, nt = np.unique(target_cls, return_counts=True)
    ap = np.zeros((len(classes), tp.shape[1]))
    p, r = np.zeros(len(classes)), np.zeros(len(classes))
    for ci, c in enumerate(classes):
        sel = pred_cls == c
        if sel.sum() == 0 or nt[ci] == 0:
            continue
        tpc, fpc = tp[sel].cumsum(0), (1 - tp[sel]).cumsum(0)
        recall, precision = tpc / (nt[ci] + eps), tpc / (tpc + fpc)
        r[ci], p[ci] = recall[-1, 0], precision[-1, 0]
        for j in range(tp.shape[1]):
            ap[ci, j] = compute_ap(recall[:, j], precision[:, j])[0]
    f1 = 2 * p * r / (p + r + eps)
    return p, r, ap, f1, classes.astype(int)


class ConfusionMatrix:
    """Detection confusion matrix with a background row / column (reference: metrics.py:114-169; val_nuclei.py:123 builds one per
    task).  matrix[predicted class, true class]; index nc = background (a missed label counts in row nc, a detection that matched
    nothing in column nc).  Matching: pairs with IoU > iou_thres; every detection keeps its best label, then every label its best
    detection."""

    def __init__(self, nc, conf=0.25, iou_thres=0.45):
        self.matrix = np.zeros((nc + 1, nc + 1))
        self.nc, self.conf, self.iou_thres = nc, conf, iou_thres

    def process_batch(self, detections, labels):
        """detections (n, 6) x1, y1, x2, y2, conf, class; labels (m, 5) class, x1, y1, x2, y2."""
        detections = detections[detections[:, 4] > self.conf]
        true_cls = labels[:, 0].int().tolist()
        det_cls = detections[:, 5].int().tolist()
        iou = box_iou(labels[:, 1:].float().cpu(), detections[:, :4].float().cpu()).numpy()       # (labels, detections)
        li, di = np.nonzero(iou > self.iou_thres)
        order = np.argsort(-iou[li, di], kind='stable')
        label_of = {}                                   # detection -> its best label
        for k in order:
            label_of.setdefault(int(di[k]), (int(li[k]), float(iou[li[k], di[k]])))
        det_of = {}                                     # label -> its best detection among those
        for d, (l, v) in sorted(label_of.items(), key=lambda kv: -kv[1][1]):
            det_of.setdefault(l, d)
        for l, c in enumerate(true_cls):
            if l in det_of:
                self.matrix[det_cls[det_of[l]], c] += 1
            else:
                self.matrix[self.nc, c] += 1
        if det_of:                                      # (with no match at all the reference counts no unmatched detections)
            used = set(det_of.values())
            for d, c in enumerate(det_cls):
                if d not in used:
                    self.matrix[c, self.nc] += 1

    def tp_fp(self):
        tp = self.matrix.diagonal()
        return tp[:-1], (self.matrix.sum(1) - tp)[:-1]


def summarize_precision_recall(stats_list, labels_text):
    """Pool per-image rows {label: (n_matched, n_true, n_pred, mean IoU)} into per-label precision / recall / F1 / mean IoU
    (reference: metrics.py:601-616)."""
    pooled = {}
    for stat in stats_list:
        for k, v in stat.items():
            pooled.setdefault(k, []).append(v)
    out = {}
    for k, rows in pooled.items():
        rows = np.array(rows)
        matched, n_true, n_pred = rows[:, 0].sum(), rows[:, 1].sum(), rows[:, 2].sum()
        precision = matched / n_pred if n_pred > 0 else np.nan
        recall = matched / n_true if n_true > 0 else np.nan
        out[labels_text[k]] = {'precision': precision, 'recall': recall, 'f1': 2 * precision * recall / (precision + recall),
                               'miou': rows[:, 3].mean()}
    return out


def get_mask_ious(a, b):
    """Mask IoU of every pair, (len(a), len(b)) fp32: a, b (n, H, W) masks on the host.  The reference's utils_nucls.get_mask_ious (:480-489)
    builds the dense (n_a, n_b, H * W) product; this is the same quotient inter / (sum(a + b) - inter + 1e-8) with the two sums taken as
    one matrix product and two row sums.  For 0 / 1 masks below 2^24 pixels every sum is an exact integer in fp32 whatever its order, so
    the result is bit-identical to the reference's (tests/golden/mask_ap.npz); soft masks agree to rounding."""
    a, b = a.detach().float().cpu().flatten(1), b.detach().float().cpu().flatten(1)
    inter = a @ b.T
    union = (a.sum(1)[:, None] + b.sum(1)[None]) - inter + 1e-8
    return inter / union


def ap_curves(hit, scores, y_pred, y_true, iouv, ignore, eps=1e-16):
    """Precision / recall / AP curves from per-prediction hit flags: the second half of APMeter.ap_per_class, shared with DeviceAPMeter.
    hit (n, n_iou) bool, scores / y_pred (n,) of the predictions that stay in the curves, y_true (n_true,), ignore a list of labels."""
    order = np.argsort(-scores, kind='stable')
    hit, scores, y_pred = hit[order], scores[order], y_pred[order]

    px = np.linspace(0, 1, 1000)
    out = {'labels': [], 'counts': [], 'px': px}
    py, ap, p, r = [], [], [], []
    for c, n_true in zip(*np.unique(y_true, return_counts=True)):
        if c in ignore:
            continue
        out['labels'].append(c)
        out['counts'].append(n_true)
        sel = y_pred == c
        if sel.sum() == 0 or n_true == 0:
            ap.append(np.zeros(len(iouv)))
            for curve in (r, p, py):
                curve.append(np.zeros(len(px)))
            continue
        tpc, fpc = hit[sel].cumsum(0), (~hit[sel]).cumsum(0)
        # fp32 curves, as the reference's torch arithmetic produces them: with fp64 a recall of exactly k/n can land ON a
        # knot of compute_ap's 101-point grid where the fp32 value falls just beside it, and the AP moves in the 4th digit
        tp32 = tpc.astype(np.float32)
        recall, precision = tp32 / np.float32(n_true + eps), tp32 / (tpc + fpc).astype(np.float32)
        r.append(np.interp(-px, -scores[sel], recall[:, 0], left=0))
        p.append(np.interp(-px, -scores[sel], precision[:, 0], left=1))
        row = np.zeros(len(iouv))
        for j in range(len(iouv)):
            row[j], mpre, mrec = compute_ap(recall[:, j], precision[:, j])
            if j == 0:
                py.append(np.interp(px, mrec, mpre))
        ap.append(row)
    stack = lambda rows, w: np.stack(rows) if rows else np.zeros((0, w))   # noqa: E731
    out.update(py=stack(py, len(px)), ap=stack(ap, len(iouv)), p=stack(p, len(px)), r=stack(r, len(px)))
    out['f1'] = 2 * out['p'] * out['r'] / (out['p'] + out['r'] + eps)
    return out


SEG_COUNT_KEYS = ('tp', 'fp', 'fn', 'iou_sum', 'C', 'U', 'inter_sum', 'pred_sum', 'true_sum')     # what pools by addition


def segmentation_counts(pairs, pred_area, true_area, pred_labels=None, true_labels=None, nc=None):
    """The counts behind PQ, AJI and Dice of two disjoint instance segmentations, from their sparse overlap as ops.label_overlap returns it:
    pairs (n, 3) int64 rows (p, t, inter > 0) sorted by (p, t), pred_area / true_area the pixels per row.  An instance is a row with
    area > 0.  Torch tensor ops on the device of `pairs` (CPU included): no host read, no loop over rows.  Returns 0-dim tensors, int64
    unless noted:
      inter_sum, pred_sum, true_sum   Dice = 2 inter_sum / (pred_sum + true_sum)
      tp, fp, fn, iou_sum (float64)   PQ (Kirillov et al. 2019): a pair with IoU > 0.5, decided as 3 inter > area_p + area_t, is unique for
                                      both of its rows; iou_sum adds inter / (area_p + area_t - inter) over them; fp / fn are the instances
                                      of either side in no such pair.  DQ = tp / (tp + fp / 2 + fn / 2), SQ = iou_sum / tp, PQ = DQ SQ
      C, U                            AJI = C / U (Kumar et al. 2017; a prediction may serve several truths): every truth with a pair takes
                                      the pair of highest IoU, ties to the lowest p, and adds its intersection to C and its union to U;
                                      a truth without a pair adds its area to U, and so does every prediction that no truth took.  IoUs are
                                      compared exactly, inter union' against inter' union in int64 (areas below 2^31: products below 2^63)
    With both label arrays (one label per row) also tp_c, fp_c, fn_c and iou_sum_c, (nc,) tensors for classes 1..nc: a pair counts for
    class c when both labels are c, fp_c / fn_c are the instances of label c not counted in tp_c.  nc=None takes the largest label, which
    is a host read.  All of them pool over images by addition (SEG_COUNT_KEYS); segmentation_ratios forms the quotients."""
    dev = pairs.device
    p, t, inter = pairs[:, 0], pairs[:, 1], pairs[:, 2]
    pa, ta = pred_area.reshape(-1).to(torch.int64), true_area.reshape(-1).to(torch.int64)
    n, n_pred, n_true = pairs.shape[0], pa.numel(), ta.numel()
    ap, at = pa[p], ta[t]
    union = ap + at - inter
    is_tp = 3 * inter > ap + at
    iou = inter.double() / union.double()
    tp = is_tp.sum()
    out = {'tp': tp, 'fp': (pa > 0).sum() - tp, 'fn': (ta > 0).sum() - tp, 'iou_sum': torch.where(is_tp, iou, iou.new_zeros(())).sum(),
           'inter_sum': inter.sum(), 'pred_sum': pa.sum(), 'true_sum': ta.sum()}

    # AJI: the best pair of every truth as a segmented maximum over the pairs in (t, p) order.  best[k] is the winner among the pairs of
    # k's truth in a window that ends at k; every round doubles the window (the order "higher IoU, then lower p" is total, so overlapping
    # windows do no harm).  A truth has at most n_pred pairs, which bounds the rounds by log2 of a shape: nothing is read.
    order = torch.sort(t, stable=True).indices
    ts, bp, bi, bu = t[order], p[order], inter[order], union[order]
    d = 1
    while d < min(n, n_pred):
        ci, cu, cp = bi[:-d], bu[:-d], bp[:-d]
        lhs, rhs = ci * bu[d:], bi[d:] * cu
        take = (ts[d:] == ts[:-d]) & ((lhs > rhs) | ((lhs == rhs) & (cp < bp[d:])))
        ni, nu, np_ = bi.clone(), bu.clone(), bp.clone()
        ni[d:], nu[d:], np_[d:] = torch.where(take, ci, bi[d:]), torch.where(take, cu, bu[d:]), torch.where(take, cp, bp[d:])
        bi, bu, bp = ni, nu, np_
        d *= 2
    last = torch.ones((n,), dtype=torch.int64, device=dev)          # the last pair of a truth holds the winner of all its pairs
    last[:-1] = (ts[1:] != ts[:-1]).to(torch.int64)
    taken = torch.zeros((n_pred,), dtype=torch.int64, device=dev).index_add_(0, bp, last) > 0
    paired = torch.zeros((n_true,), dtype=torch.int64, device=dev).index_add_(0, t, torch.ones_like(t)) > 0
    out['C'] = (bi * last).sum()
    out['U'] = (bu * last).sum() + (ta * ~paired).sum() + (pa * ~taken).sum()

    if pred_labels is not None and true_labels is not None:
        lp, lt = pred_labels.reshape(-1).to(dev, torch.int64), true_labels.reshape(-1).to(dev, torch.int64)
        if nc is None:
            nc = int(max(lp.max() if n_pred else 0, lt.max() if n_true else 0, 0))
        per_class = lambda labels, weight: torch.zeros((nc + 1,), dtype=weight.dtype, device=dev).index_add_(   # noqa: E731
            0, torch.where((labels >= 1) & (labels <= nc), labels, torch.zeros_like(labels)), weight)[1:]
        both = is_tp & (lp[p] == lt[t])
        tp_c = per_class(lp[p], both.to(torch.int64))
        out.update(tp_c=tp_c, fp_c=per_class(lp, (pa > 0).to(torch.int64)) - tp_c, fn_c=per_class(lt, (ta > 0).to(torch.int64)) - tp_c,
                   iou_sum_c=per_class(lp[p], torch.where(both, iou, iou.new_zeros(()))))
    return out


def segmentation_counts_to_host(counts):
    """a dict of device tensors (segmentation_counts, or sums of it) as Python ints / floats and numpy arrays, through ONE copy"""
    if not counts:
        return {}
    flat = torch.cat([v.reshape(-1) if v.dtype == torch.int64 else v.reshape(-1).double().view(torch.int64) for v in counts.values()]).cpu().numpy()
    out, at = {}, 0
    for k, v in counts.items():
        part = flat[at:at + v.numel()]
        at += v.numel()
        part = part if v.dtype == torch.int64 else part.view(np.float64)
        out[k] = part.copy() if v.dim() else (int(part[0]) if v.dtype == torch.int64 else float(part[0]))
    return out


def segmentation_ratios(c):
    """PQ / SQ / DQ / AJI / Dice (and mPQ when the per-class counts are there) from host counts; a ratio with denominator 0 is 0.0, as
    val_nuclei.summarize_stats reports an empty meter.  mPQ is the mean of PQ_c over the classes with an instance on either side."""
    div = lambda a, b: float(a) / float(b) if b else 0.0   # noqa: E731
    dq, sq = div(c['tp'], c['tp'] + 0.5 * c['fp'] + 0.5 * c['fn']), div(c['iou_sum'], c['tp'])
    out = {'pq': dq * sq, 'sq': sq, 'dq': dq, 'aji': div(c['C'], c['U']), 'dice': div(2 * c['inter_sum'], c['pred_sum'] + c['true_sum'])}
    if 'tp_c' in c:
        pq_c = [div(i, tp + 0.5 * fp + 0.5 * fn) for i, tp, fp, fn in zip(c['iou_sum_c'], c['tp_c'], c['fp_c'], c['fn_c']) if tp + fp + fn > 0]
        out['mpq'] = sum(pq_c) / len(pq_c) if pq_c else 0.0
    return out


class APMeter:
    """Dataset-level detection AP with the reference's accumulation and matching rules (metayolo/models/metrics.py:251-375).

    add(): per image, predictions are put in descending score order; every (prediction, truth) pair with IoU >= 0.5 is recorded
    with dataset-global indices, the image's pairs in descending IoU order.
    ap_per_class(): pairs touching an ignored label are dropped; each prediction keeps its first (= best-IoU) pair, then each
    truth keeps the pair of its lowest-index (= best-score) prediction; a pair counts only when the two labels agree; a
    prediction is a true positive at threshold t when its pair's IoU >= t.  Predictions whose only pairs were with ignored
    truths are removed from the precision/recall curves.  Returns the reference's stats dict:
    'labels', 'counts', 'px', 'py' (n_cls, 1000), 'ap' (n_cls, n_iou), 'p', 'r', 'f1' (n_cls, 1000).
    Host-side numpy with a dense IoU matrix per image: for tiles.  DeviceAPMeter computes the same on the device.
    add(..., iou_type='masks') with dense 0 / 1 'masks' on both sides takes the IoU from get_mask_ious instead of the boxes.
    Tie rule: equal scores inside one image are ranked by torch.sort, whose order among ties is unspecified; DeviceAPMeter ranks the lower
    row first.  This is the one place the two meters may differ."""

    def __init__(self, labels_text={}):
        self.iouv = np.linspace(0.5, 0.95, 10)
        self.labels_text = labels_text
        self.reset()

    def reset(self):
        self.n_pred = self.n_true = 0
        self._scores, self._y_pred, self._y_true = [], [], []
        self._m_pred, self._m_true, self._ious = [], [], []

    # the reference exposes these as tensors; keep the names readable from outside
    @property
    def scores(self):
        return np.concatenate(self._scores) if self._scores else np.zeros(0, np.float32)

    @property
    def y_pred(self):
        return np.concatenate(self._y_pred) if self._y_pred else np.zeros(0, np.int64)

    @property
    def y_true(self):
        return np.concatenate(self._y_true) if self._y_true else np.zeros(0, np.int64)

    @property
    def n_match(self):
        return int(sum(len(v) for v in self._ious))

    def add(self, output, target, iou_type='boxes'):
        scores, order = torch.sort(output['scores'].detach().float().cpu(), descending=True)
        labels = output['labels'].detach().cpu()[order]
        tlabels = target['labels'].detach().cpu()
        n_pred, n_true = len(scores), len(tlabels)
        if not (n_pred and n_true):
            iou = np.zeros((n_pred, n_true), np.float32)
        elif iou_type == 'masks' and 'masks' in output and 'masks' in target:
            # dense 0 / 1 masks (n, H, W) or (n, 1, H, W) on both sides, as the reference intends (metrics.py:274-275)
            iou = get_mask_ious(output['masks'].detach().cpu()[order], target['masks'].detach().cpu()).numpy()
        else:
            iou = box_iou(output['boxes'].detach().float().cpu()[order], target['boxes'].detach().float().cpu()).numpy()
        pi, ti = np.nonzero(iou >= self.iouv.min())
        v = iou[pi, ti]
        o = np.argsort(-v, kind='stable')
        self._m_pred.append(pi[o] + self.n_pred)
        self._m_true.append(ti[o] + self.n_true)
        self._ious.append(v[o].astype(np.float32))
        self._y_true.append(tlabels.numpy().astype(np.int64))
        self._y_pred.append(labels.numpy().astype(np.int64))
        self._scores.append(scores.numpy())
        self.n_pred += n_pred
        self.n_true += n_true

    def ap_per_class(self, iouv=None, ignore=(-100, -1), eps=1e-16):
        # thresholds compare in fp32, as with the torch.linspace the reference's caller passes (val_nuclei.py:56)
        iouv = np.asarray(self.iouv if iouv is None else iouv, dtype=np.float32)
        cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)   # noqa: E731
        m_pred, m_true, ious = cat(self._m_pred, np.int64), cat(self._m_true, np.int64), cat(self._ious, np.float32)
        y_true, y_pred, scores = self.y_true, self.y_pred, self.scores
        ignore = list(ignore) if ignore else []

        ignored = (np.isin(y_true[m_true], ignore) | np.isin(y_pred[m_pred], ignore)) if ignore else np.zeros(len(m_pred), bool)
        k_pred, k_true, k_iou = m_pred[~ignored], m_true[~ignored], ious[~ignored]
        first = np.unique(k_pred, return_index=True)[1]            # one pair per prediction: its first = highest IoU
        k_pred, k_true, k_iou = k_pred[first], k_true[first], k_iou[first]
        first = np.unique(k_true, return_index=True)[1]            # one pair per truth: lowest prediction index
        k_pred, k_true, k_iou = k_pred[first], k_true[first], k_iou[first]
        agree = y_true[k_true] == y_pred[k_pred]
        k_pred, k_iou = k_pred[agree], k_iou[agree]
        hit = np.zeros((self.n_pred, len(iouv)), dtype=bool)
        hit[k_pred] = k_iou[:, None] >= iouv[None]

        if ignored.any():
            live = np.ones(self.n_pred, dtype=bool)
            live[np.setdiff1d(m_pred[ignored], k_pred)] = False
            hit, scores, y_pred = hit[live], scores[live], y_pred[live]
        return ap_curves(hit, scores, y_pred, y_true, iouv, ignore, eps)


class DeviceAPMeter:
    """APMeter with the matching on the device (ops.ap_match, csrc/score.hip): no pair list, no sort, no dense IoU matrix on the host.

    add_batch(outputs, targets): `outputs` is what Model.forward delivers for one task of a batch, a list of per-image dicts
    {'boxes', 'scores', 'labels'} of device tensors, or the compacted (boxes, scores, labels, n_keep[, masks]) tuple of device_outputs=True;
    `targets` a list of per-image dicts {'boxes', 'labels'}.  The batch is concatenated on the device, matched in one call, and its result
    tensors stay on the device: no device-to-host read per image or per batch.  add(output, target) is a batch of one.
    ap_per_class() copies the compact arrays (scores, labels, hit bits, live flags) to the host once and returns APMeter's stats dict through
    the same curve arithmetic (ap_curves).  iouv (at most 16 thresholds) and ignore (at most 4 labels) are fixed at construction, because the
    hit bits are made at add time: passing different ones to ap_per_class raises ValueError.  Multi-label (2-D) outputs are flattened by the
    caller (val_nuclei.flatten_onehot_objects).
    Tie rule: equal scores inside one image are ranked lower row first; APMeter ranks them by torch.sort, whose order among ties is
    unspecified.  This is the one place the two meters may differ.  The properties list predictions per image in descending score order, as
    APMeter's do."""

    def __init__(self, labels_text={}, iouv=torch.linspace(0.5, 0.95, 10), ignore=(-100, -1)):
        self.iouv = np.asarray(iouv.tolist() if hasattr(iouv, 'tolist') else list(iouv), dtype=np.float32)
        self.ignore = tuple(int(v) for v in (ignore or ()))
        from ... import ops
        if not 1 <= len(self.iouv) <= ops.AP_MAX_IOU or len(self.ignore) > ops.AP_MAX_IGNORE:
            raise ValueError(f'DeviceAPMeter: 1 to {ops.AP_MAX_IOU} IoU thresholds and at most {ops.AP_MAX_IGNORE} ignored labels')
        self.labels_text = labels_text
        self.reset()

    def reset(self):
        self._batches = []          # per batch: device tensors (scores, labels, hit, live, pred_off, true_labels, true_off)
        self._host_cache = None
        self._seg = None            # add_batch_masks: the pooled segmentation_counts, device tensors

    def add(self, output, target, iou_type='boxes'):
        if iou_type == 'masks' and 'masks' in output and 'masks' in target:
            raise NotImplementedError('mask IoU: the reference calls get_mask_ious here (metrics.py:275), a function its metrics module neither defines nor imports')
        self.add_batch([output], [target])

    @staticmethod
    def _offsets(dicts, key, dev):
        """int32 prefix offsets of the per-image rows under `key`, on the device (lengths are host values: an upload, no read)"""
        return torch.tensor(np.concatenate(([0], np.cumsum([len(d[key]) for d in dicts]))), dtype=torch.int32, device=dev)

    @staticmethod
    def _cat(dicts, key, dev, dtype=torch.int64):
        """the per-image tensors under `key` as one flat tensor of `dtype` on the device"""
        return torch.cat([d[key].detach().reshape(-1).to(dtype) for d in dicts]).to(dev)

    def _store(self, scores, labels, hit, live, pred_off, tlabels, true_off):
        self._batches.append((scores, labels, hit, live, pred_off, tlabels, true_off))
        self._host_cache = None

    def add_batch(self, outputs, targets, info=None):
        from ... import ops
        if isinstance(outputs, tuple):
            boxes, scores, labels, n_keep = outputs[:4]          # (a fifth element: the batch's compact masks, not scored here)
            dev = boxes.device
            pred_off = torch.zeros((n_keep.numel() + 1,), dtype=torch.int32, device=dev)
            pred_off[1:] = torch.cumsum(n_keep.to(torch.int32), 0)
        else:
            if not len(outputs):
                return
            if outputs[0]['labels'].dim() != 1:
                raise ValueError('DeviceAPMeter: multi-label outputs must be flattened by the caller (val_nuclei.flatten_onehot_objects)')
            dev = outputs[0]['boxes'].device
            boxes = torch.cat([o['boxes'].detach().float().reshape(-1, 4) for o in outputs])
            scores, labels = self._cat(outputs, 'scores', dev, torch.float32), self._cat(outputs, 'labels', dev)
            pred_off = self._offsets(outputs, 'scores', dev)
        if len(targets) != pred_off.numel() - 1:
            raise ValueError(f'DeviceAPMeter: {pred_off.numel() - 1} images of predictions, {len(targets)} of truths')
        tboxes = torch.cat([t['boxes'].detach().float().reshape(-1, 4) for t in targets]).to(dev)
        tlabels, true_off = self._cat(targets, 'labels', dev), self._offsets(targets, 'labels', dev)
        hit, live, _, _ = ops.ap_match(boxes, scores, labels, pred_off, tboxes, tlabels, true_off, self.iouv, ignore=self.ignore, info=info)
        self._store(scores.detach().float().reshape(-1), labels.detach().reshape(-1).to(torch.int64), hit, live, pred_off, tlabels, true_off)

    def add_batch_masks(self, outputs, targets, size, threshold=0.5, max_pairs=None):
        """A batch scored on mask IoU (ops.label_overlap + ops.mask_ap_match, csrc/mask_score.hip).  `outputs`: per-image dicts with 'boxes',
        'scores', 'labels' and 'masks' (R, 1, M, M), rows in descending score order as the model delivers them (the mask paste gives a pixel
        to the lowest row that covers it); `targets`: per-image dicts with 'labels' and 'instances', an (H, W) = size map holding the index of
        the object that owns each pixel (uint16 with 0xFFFF background, as the tile bank stores it, or int32 with negative background).  Per
        image one ops.paste_label_map into its slice of a (B, H, W) map, then one overlap launch over the batch with per-image row bases and
        one matching call.  Instances are disjoint on both sides by construction.  One device-to-host read per batch (the overlap status).
        max_pairs sizes the overlap's pair table (ops.label_overlap; default: from the row counts), for batches whose instances fragment into
        more overlapping pairs than that holds.  A 16-bit map is refused once the batch has more than 65535 truths (0xFFFF would be a row).
        Results are stored as add_batch stores them; the batch's segmentation counts (segmentation_counts) are added to the meter's on the
        device, for segmentation_summary."""
        from ... import ops
        if not len(outputs):
            return
        if len(targets) != len(outputs):
            raise ValueError(f'DeviceAPMeter: {len(outputs)} images of predictions, {len(targets)} of truths')
        if outputs[0]['labels'].dim() != 1:
            raise ValueError('DeviceAPMeter: multi-label outputs must be flattened by the caller (val_nuclei.flatten_onehot_objects)')
        H, W = int(size[0]), int(size[1])
        dev = outputs[0]['scores'].device
        pred_off, true_off = self._offsets(outputs, 'scores', dev), self._offsets(targets, 'labels', dev)
        n_true = int(sum(len(t['labels']) for t in targets))
        pred_map = torch.empty((len(outputs), H, W), dtype=torch.int32, device=dev)
        true_map = torch.empty((len(outputs), H, W), dtype=torch.int32, device=dev)
        for i, (o, t) in enumerate(zip(outputs, targets)):
            ops.paste_label_map(o['masks'], o['boxes'], (H, W), threshold=threshold, out=pred_map[i])
            inst = t['instances']
            if tuple(inst.shape) != (H, W):
                raise ValueError(f"DeviceAPMeter: 'instances' of image {i} is {tuple(inst.shape)}, the canvas {(H, W)}")
            true_map[i] = ops._label_map_i32('add_batch_masks', inst.to(dev), 'instances', n_true)
        scores, labels, tlabels = self._cat(outputs, 'scores', dev, torch.float32), self._cat(outputs, 'labels', dev), self._cat(targets, 'labels', dev)
        pairs, pa, ta = ops.label_overlap(pred_map, true_map, scores.numel(), tlabels.numel(), seg=(pred_off[:-1], true_off[:-1]), max_pairs=max_pairs)
        hit, live, _, _ = ops.mask_ap_match(pairs, pa, ta, scores, labels, tlabels, self.iouv, ignore=self.ignore)
        self._store(scores, labels, hit, live, pred_off, tlabels, true_off)
        counts = segmentation_counts(pairs, pa, ta)                  # rows of different images share no pair: the batch is one pooled image
        self._seg = counts if self._seg is None else {k: self._seg[k] + v for k, v in counts.items()}

    def segmentation_summary(self):
        """PQ / SQ / DQ / AJI / Dice of everything add_batch_masks received, as segmentations (segmentation_counts: class-agnostic, every
        row that owns a pixel is an instance): the ratios of the pooled counts, not means of per-image ratios, and the counts themselves
        (SEG_COUNT_KEYS).  One device-to-host copy.  Without any add_batch_masks call: all zero."""
        c = segmentation_counts_to_host(self._seg) if self._seg is not None else {k: 0.0 if k == 'iou_sum' else 0 for k in SEG_COUNT_KEYS}
        return {**segmentation_ratios(c), **c}

    def _host(self):
        """the compact arrays on the host (one copy per array), rows outside every image's span dropped, and the image of every prediction"""
        if self._host_cache is None:
            z = lambda dt: np.zeros(0, dt)   # noqa: E731
            if not self._batches:
                self._host_cache = (z(np.float32), z(np.int64), z(np.uint16), z(bool), z(np.int64), z(np.int64))
                return self._host_cache
            cat = lambda k: torch.cat([b[k] for b in self._batches]).cpu().numpy()   # noqa: E731
            scores, y_pred, hit, live, y_true = cat(0), cat(1), cat(2).view(np.uint16), cat(3).astype(bool), cat(5)
            poffs, toffs = [b[4].cpu().numpy().astype(np.int64) for b in self._batches], [b[6].cpu().numpy().astype(np.int64) for b in self._batches]
            keep_p, keep_t, image, base_p, base_t, n_img = [], [], [], 0, 0, 0
            for b, po, to in zip(self._batches, poffs, toffs):
                keep_p.append(base_p + np.arange(po[0], po[-1]))
                keep_t.append(base_t + np.arange(to[0], to[-1]))
                image.append(n_img + np.repeat(np.arange(len(po) - 1), np.diff(po)))
                base_p, base_t, n_img = base_p + len(b[0]), base_t + len(b[5]), n_img + len(po) - 1
            kp, kt = np.concatenate(keep_p), np.concatenate(keep_t)
            self._host_cache = (scores[kp], y_pred[kp], hit[kp], live[kp], y_true[kt], np.concatenate(image))
        return self._host_cache

    def _ranked(self):
        scores, _, _, _, _, image = self._host()
        return np.lexsort((np.arange(len(scores)), -scores, image))      # per image, descending score, lower row first

    @property
    def n_pred(self):
        return len(self._host()[0])

    @property
    def n_true(self):
        return len(self._host()[4])

    @property
    def scores(self):
        return self._host()[0][self._ranked()]

    @property
    def y_pred(self):
        return self._host()[1][self._ranked()]

    @property
    def y_true(self):
        return self._host()[4]

    def ap_per_class(self, iouv=None, ignore=None, eps=1e-16):
        if iouv is not None:
            given = np.asarray(iouv.tolist() if hasattr(iouv, 'tolist') else list(iouv), dtype=np.float32)
            if given.shape != self.iouv.shape or not np.array_equal(given, self.iouv):
                raise ValueError('DeviceAPMeter: the IoU thresholds are fixed at construction (the hit bits are made at add time)')
        if ignore is not None and sorted(int(v) for v in ignore) != sorted(self.ignore):
            raise ValueError('DeviceAPMeter: the ignored labels are fixed at construction (the matching is made at add time)')
        scores, y_pred, bits, live, y_true, _ = self._host()
        hit = ((bits[:, None] >> np.arange(len(self.iouv), dtype=np.uint16)[None]) & 1).astype(bool)
        if not live.all():
            hit, scores, y_pred = hit[live], scores[live], y_pred[live]
        return ap_curves(hit, scores, y_pred, y_true, self.iouv, list(self.ignore), eps)
