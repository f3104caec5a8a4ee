"""Plain numpy restatement of csrc/detect.hip's arithmetic kernels (hdy_decode, hdy_det_outputs, hdy_det_grad_pack): no torch and no
hd_yolo_amd in the arithmetic.  tests/test_detect_ref_host.py pins it to the reference's own decode outputs (tests/golden/decode.npz) and to
the eager tensor expressions of Detect.compute_outputs on the CPU; tests/test_gpu_detect_direct.py compares the kernels with it.  NMS has no
restatement here: oracle/nms_ref.c is the oracle and oracle.nms_ref's numpy functions the second opinion; `nms_expected` only gathers the
rows the oracle kept.

decode.  float64 from the fp32 logits: s = 1 / (1 + exp(-x)) (an overflowing exp gives s = 0, NaN gives NaN), then per candidate (a, y, x)
    [(2s - 0.5 + gx) stride, (2s - 0.5 + gy) stride, (2s)^2 aw, (2s)^2 ah, s, s, ..., level id]
rows in (a, y, x) order.  `decode(..., dtype=np.float32)` rounds the same expression in fp32 operation by operation, as the kernels write
it (numpy's exp and division instead of v_exp_f32 and v_rcp_f32): the CPU column of the GPU file's table.

decode_bound.  The kernels' sigmoid is v_rcp_f32(1 + v_exp_f32(-x log2 e)).  With both instructions at 1 ulp (the assumption in the
kernel's comment), the argument t = -x log2 e rounded once in fp32 (|t| 2^-24 absolute, a factor exp(|t| 2^-24 ln 2) = 1 + |x| 2^-24 on
the power; log2 e itself is rounded: another |x| 2^-24), 1 ulp = 2^-23 for v_exp_f32 (it reaches s scaled by e / (1 + e) <= 1), the sum
1 + e rounded once (2^-24) and 1 ulp = 2^-23 for v_rcp_f32:
    relative error of s  <=  (2 |x| + 2 + 1 + 2) 2^-24  <  (2 |x| + 6) 2^-24.
It is used for REPORTING only (`decode_units` spreads it over the output columns); the asserted tolerance is the project's 1e-4.

det_outputs.  fp32, statement by statement: child *= parent over the pairs in order on the first n_keep[b] rows of each image, then
either all 1 + nc scores with (score > conf) flags, or the best class (first maximum; a NaN among the class scores IS the maximum and the
first NaN its position, as torch.max) with the objectness fallback and label -100; rows compacted over the batch, offsets = prefix sums.

grad_pack.  (b, a, y, x, o) -> [B, ny, nx, ldo] with channel a no + o, +0 beyond na no, rounded to bf16 by round-to-nearest-even.
"""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126                 # smallest normal fp32: the floor that allows a flushed subnormal


def q_bf16(a):
    """fp32 -> the nearest bf16 value (ties to even) as fp32; NaN and infinities kept"""
    a = np.ascontiguousarray(a, np.float32)
    u = a.view(np.uint32).astype(np.uint64)
    u = ((u + 0x7fff + ((u >> 16) & 1)) >> 16) << 16
    out = u.astype(np.uint32).view(np.float32)
    return np.where(np.isfinite(a), out, a)


# ------------------------------------------------------------------------------------------ decode
def sigmoid(x, dtype=np.float64):
    x = np.asarray(x, np.float32).astype(dtype)
    with np.errstate(over='ignore', invalid='ignore'):
        return dtype(1) / (dtype(1) + np.exp(-x))          # exp overflow -> inf -> 0; NaN -> NaN


def decode(det, anchors_px, stride, level_id, dtype=np.float64):
    """det (B, na, ny, nx, no) fp32 logits -> (B, na ny nx, no + 1) of `dtype`"""
    det = np.asarray(det, np.float32)
    B, na, ny, nx, no = det.shape
    f = dtype
    s = sigmoid(det, f)
    anc = np.asarray(anchors_px, np.float32).astype(f).reshape(na, 2)
    gx = np.arange(nx, dtype=f).reshape(1, 1, 1, nx)
    gy = np.arange(ny, dtype=f).reshape(1, 1, ny, 1)
    st = f(np.float32(stride))
    out = np.empty((B, na, ny, nx, no + 1), f)
    with np.errstate(invalid='ignore'):
        out[..., 0] = (s[..., 0] * f(2) - f(0.5) + gx) * st
        out[..., 1] = (s[..., 1] * f(2) - f(0.5) + gy) * st
        q2, q3 = s[..., 2] * f(2), s[..., 3] * f(2)
        out[..., 2] = q2 * q2 * anc[:, 0].reshape(1, na, 1, 1)
        out[..., 3] = q3 * q3 * anc[:, 1].reshape(1, na, 1, 1)
    out[..., 4:no] = s[..., 4:]
    out[..., no] = f(level_id)
    return out.reshape(B, na * ny * nx, no + 1)


def decode_bound(x):
    """relative error the kernels' sigmoid may have at logit x under the 1-ulp assumptions (module docstring)"""
    return (2.0 * np.abs(np.asarray(x, np.float64)) + 6.0) * U


def decode_units(det, anchors_px, stride):
    """decode_bound carried to the output columns, (B, na ny nx, no): what one 'unit' of error is for each element.
    score: s b.  w, h = (2s)^2 a: twice the relative error of s plus the roundings of q q and of the product with the anchor.
    x, y = (2s - 0.5 + g) stride: 2 s b from the sigmoid, the rounding of 2s - 0.5 (one, the product is exact), of the sum and of the product."""
    det = np.asarray(det, np.float32)
    B, na, ny, nx, no = det.shape
    ref = decode(det, anchors_px, stride, 0)[..., :no].reshape(B, na, ny, nx, no)
    s = sigmoid(det)
    b = decode_bound(det)
    with np.errstate(invalid='ignore'):
        unit = np.abs(s) * b
        unit[..., 2:4] = np.abs(ref[..., 2:4]) * (2.0 * b[..., 2:4] + 2.0 * U)
        st = float(np.float32(stride))
        unit[..., 0:2] = st * (2.0 * s[..., 0:2] * b[..., 0:2] + U * np.abs(2.0 * s[..., 0:2] - 0.5)) + 2.0 * U * np.abs(ref[..., 0:2])
    return unit.reshape(B, na * ny * nx, no)


def decode_error_in_units(got, det, anchors_px, stride):
    """|got - ref| / unit over the elements whose reference is finite and whose score / size is a normal fp32 number (below that the
    hardware may flush and the absolute floor of the assertion applies); returns the flat array of ratios"""
    det = np.asarray(det, np.float32)
    no = det.shape[-1]
    ref = decode(det, anchors_px, stride, 0)[..., :no]
    unit = decode_units(det, anchors_px, stride)
    with np.errstate(invalid='ignore', divide='ignore'):
        ok = np.isfinite(ref) & (unit > 0)
        ok[..., 2:] &= np.abs(ref[..., 2:]) >= TINY
        r = np.abs(np.asarray(got, np.float64)[..., :no] - ref) / unit
    return r[ok]


# ------------------------------------------------------------------------------------------ NMS (gathering only)
def nms_expected(preds, nc, conf, iou, max_det, min_wh=2.0, class_aware=False):
    """oracle/nms_ref.c's kept rows and what hdy_nms_batched gathers for them: boxes (xywh2xyxy in fp32), the 1 + nc scores, the extra
    columns, the ranking score and the best class"""
    from oracle import nms_ref
    preds = np.ascontiguousarray(preds, np.float32)
    B, N, row = preds.shape
    keep, n_keep, cls = nms_ref.nms_batched_c(preds, nc, conf, iou, max_det, min_wh=min_wh, class_aware=class_aware)
    out = {'keep': keep, 'n_keep': n_keep, 'cls': cls, 'boxes': [], 'scores': [], 'extra': [], 'conf': []}
    for b in range(B):
        r = preds[b][keep[b, :n_keep[b]]]
        with np.errstate(invalid='ignore', over='ignore'):
            out['boxes'].append(nms_ref.xywh2xyxy_np(r[:, :4]) if len(r) else np.zeros((0, 4), np.float32))
            out['scores'].append(r[:, 4:5 + nc])
            out['extra'].append(r[:, 5 + nc:])
            out['conf'].append(best_class(r, nc)[0] if class_aware else r[:, 4])
    return out


def best_class(rows, nc):
    """score = obj * cls in fp32, first strict maximum (a NaN product never replaces the best and a NaN first product is never replaced: the
    oracle's loop)"""
    rows = np.asarray(rows, np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        v = rows[:, 5:5 + nc] * rows[:, 4:5]
    best, arg = v[:, 0].copy(), np.zeros(len(rows), np.int32)
    for k in range(1, nc):
        with np.errstate(invalid='ignore'):
            m = v[:, k] > best
        best[m], arg[m] = v[m, k], k
    return best, arg


# ------------------------------------------------------------------------------------------ det_outputs
def det_outputs(scores, boxes, n_keep, pairs, conf, multi_label):
    """scores (B, max_det, 1 + nc), boxes (B, max_det, 4), n_keep (B,), pairs [(child, parent), ...] -> dict:
    'scores_inplace' the padded scores after the products (rows beyond n_keep untouched), 'boxes' / 'scores' / 'labels' compacted to
    sum(n_keep) rows, 'offsets' (B + 1,) int32"""
    sc = np.array(scores, np.float32, copy=True)
    boxes = np.asarray(boxes, np.float32)
    n_keep = np.asarray(n_keep, np.int64)
    B, max_det, C = sc.shape
    cf = np.float32(conf)
    ob, os_, ol = [], [], []
    for b in range(B):
        x = sc[b, :n_keep[b]]
        with np.errstate(invalid='ignore', over='ignore'):
            for c, p in pairs:
                x[:, c] *= x[:, p]
            ob.append(boxes[b, :n_keep[b]])
            if multi_label:
                os_.append(x.copy())
                ol.append(x > cf)
            else:
                cls = x[:, 1:]
                arg = np.argmax(cls, 1) if len(x) else np.zeros((0,), np.int64)        # first maximum; NaN is the maximum, first NaN wins
                best = cls[np.arange(len(x)), arg]
                hit = best > cf
                os_.append(np.where(hit, best, x[:, 0]).astype(np.float32))
                ol.append(np.where(hit, arg + 1, -100).astype(np.int64))
    off = np.zeros(B + 1, np.int32)
    off[1:] = np.cumsum(n_keep)
    return {'scores_inplace': sc, 'boxes': np.concatenate(ob), 'scores': np.concatenate(os_), 'labels': np.concatenate(ol), 'offsets': off}


# ------------------------------------------------------------------------------------------ det_grad_pack
def grad_pack(g, na, no, ldo, dtype):
    """g (B, na, ny, nx, no) fp32 -> (B, ny, nx, ldo) fp32 holding the values of `dtype` ('f32' or 'bf16')"""
    g = np.asarray(g, np.float32)
    B, na_, ny, nx, no_ = g.shape
    assert (na_, no_) == (na, no) and ldo >= na * no
    out = np.zeros((B, ny, nx, ldo), np.float32)
    out[..., :na * no] = g.transpose(0, 2, 3, 1, 4).reshape(B, ny, nx, na * no)
    return q_bf16(out) if dtype == 'bf16' else out
