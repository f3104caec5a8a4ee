"""Plain numpy restatement of csrc/pool.hip (hdy_sppf_pool_fwd / _bwd, hdy_upsample2x_fwd / _bwd, hdy_stem_prep, hdy_nchw_to_nhwc): no torch
and no hd_yolo_amd in the arithmetic.  tests/test_pool_ref_host.py pins it to ATen on the CPU; tests/test_gpu_pool_direct.py compares the
kernels with it.  Tensors are NHWC arrays [N, H, W, C]; bf16 values travel as the float32 numbers they are (`q`).

SPPF forward.  Three chained 5x5 / stride 1 / padding 2 maxima.  A window is scanned in row-major order over its in-bounds elements only,
starting FROM the first of them (value and position), and the maximum is replaced when `v > best or isnan(v)` (ATen's max_pool2d; NaN
policy 'last': the last NaN of a window keeps the position) or, under policy 'first', when `v > best or (isnan(v) and not isnan(best))`
(the first NaN keeps it: what the order-preserving keys of pool.hip do).  An output is one of the inputs, bit for bit.  Per level:
    y     the maxima
    idx   ATen's flat index h' W + w' of the chosen element, from the 25-tap scan
    pos   the byte pool.hip stores, dy | dx' << 4, from the two 5-tap stages the kernels run: dx' (0..4) is the row stage's choice for the
          row maximum AT this position, dy (0..4) the column stage's choice among the five row maxima for THIS output.
`decode(pos)` maps the bytes back to flat indices: output (h, w) took row maximum (h + dy - 2, w), which took source column
w + dx'(h + dy - 2, w) - 2.  The host test asserts decode(pos) == idx on every case: the first (last, for NaNs) element in row-major order
is in the first (last) row whose row maximum equals the window's, and there the first (last) such column.

SPPF backward, float64:  dx = g0 + P1^T (g1 + P2^T (g2 + P3^T g3)),  P^T t = scatter of t to the level's indices;  A is the same expression
over |g|.  Bound: the kernel runs each P^T as a column gather of five candidates followed by a row gather of five candidates plus the
level's own gradient, all in fp32: per level at most 5 + 5 + 1 = 11 additions on the chain to one element, three levels: n = 33 (an
overcount: the first addition of each gather is onto 0 and exact, which leaves 27 roundings, so (1 + U)^27 - 1 < 33 U covers the
higher-order terms too).  Every partial sum is bounded by the same expression over |g|, hence  |dx - ref| <= 33 U A,  U = 2^-24.
bf16: the fp32 value is rounded once: 2^-8 (|ref| + bound) on top (half an ulp of 8 significand bits).  With integer-valued gradients every
partial sum is an integer below 2^24 and fp32 is exact.

Upsample (nearest, 2x).  Forward: y[n, oh, ow] = x[n, oh >> 1, ow >> 1], a copy of bits.  Backward: the float64 sum of the four sources, plus
the old value when accumulating; the kernel adds the old value and four sources in fp32 (0 + old is exact): at most 5 additions,
|dx - ref| <= 5 U A with A the sum of the magnitudes; bf16 as above.
stem_prep: [B, 3, H, W] fp32 -> [B, H + 2 pad, W + 2 pad, 4] with a zero border and a zero fourth channel, rounded to nearest even for bf16.
nchw_to_nhwc: [N, C, H, W] fp32 -> [N, H, W, C], the same rounding.
"""
import numpy as np

from segk_ref import check, f64, ratios  # noqa: F401

U = 2.0 ** -24
BF16_HALF_ULP = 2.0 ** -8
SPPF_ADDS = 33                     # 3 levels x (5 column candidates + 5 row candidates + the level's own gradient)
UP_ADDS = 5                        # old value + four sources


def q(a, dt):
    """round to the tensor type's values (bf16: nearest even on the upper 16 bits; NaN and infinities kept), as float32"""
    a = np.ascontiguousarray(a, np.float32)
    if dt == 'f32':
        return a
    u = a.view(np.uint32).astype(np.uint64)
    u = ((u + 0x7fff + ((u >> 16) & 1)) >> 16) << 16
    out = u.astype(np.uint32).view(np.float32)
    return np.where(np.isfinite(a), out, a)


def finish(bound, ref, bf16):
    """the bf16 rounding of the output on top of an fp32 bound"""
    with np.errstate(all='ignore'):
        b = f64(bound)
        return b + BF16_HALF_ULP * (np.abs(f64(ref)) + b) if bf16 else b


# ------------------------------------------------------------------------------------------ SPPF forward
def _replace(v, best, policy):
    with np.errstate(invalid='ignore'):
        return (v > best) | (np.isnan(v) if policy == 'last' else (np.isnan(v) & ~np.isnan(best)))


def _scan(x, axis, policy):
    """5 taps along `axis` (1: rows h, 2: columns w) of [N, H, W, C]: start from the first in-bounds tap -> (maximum, tap 0..4)"""
    size = x.shape[axis]
    at = np.arange(size)
    first = np.maximum(0, 2 - at)
    shape = [1, 1, 1, 1]
    shape[axis] = size
    best = np.take(x, at + first - 2, axis=axis)
    pos = np.broadcast_to(first.reshape(shape), x.shape).astype(np.uint8)
    for t in range(5):
        src = at + t - 2
        ok = ((src >= 0) & (src < size)).reshape(shape)
        v = np.take(x, np.clip(src, 0, size - 1), axis=axis)
        rep = ok & _replace(v, best, policy)
        best = np.where(rep, v, best)
        pos = np.where(rep, np.uint8(t), pos)
    return best, pos


def _scan25(x, policy):
    """ATen's scan of the whole window in row-major order -> (maximum, flat index)"""
    N, H, W, C = x.shape
    hh, ww = np.arange(H)[:, None], np.arange(W)[None, :]
    h0, w0 = np.maximum(hh - 2, 0), np.maximum(ww - 2, 0)
    best = x[:, h0, w0, :]
    idx = np.broadcast_to((h0 * W + w0)[None, :, :, None], x.shape).astype(np.int64)
    for dy in range(5):
        for dx in range(5):
            sh, sw = hh + dy - 2, ww + dx - 2
            ok = ((sh >= 0) & (sh < H) & (sw >= 0) & (sw < W))[None, :, :, None]
            v = x[:, np.clip(sh, 0, H - 1), np.clip(sw, 0, W - 1), :]
            rep = ok & _replace(v, best, policy)
            best = np.where(rep, v, best)
            idx = np.where(rep, (sh * W + sw)[None, :, :, None], idx)
    return best, idx


def pool5(x, policy='last'):
    """one 5x5 / 1 / 2 maximum of [N, H, W, C] float32 -> (y, idx, pos)"""
    x = np.ascontiguousarray(x, np.float32)
    row, dxp = _scan(x, 2, policy)
    y, dy = _scan(row, 1, policy)
    y25, idx = _scan25(x, policy)
    assert np.array_equal(y.view(np.uint32), y25.view(np.uint32)), 'row / column stages differ from the 25-tap scan'
    return y25, idx, (dy | (dxp << 4)).astype(np.uint8)


def sppf_fwd(x, policy='last'):
    """-> ([y1, y2, y3], [idx1, idx2, idx3], [pos1, pos2, pos3])"""
    ys, idxs, poss = [], [], []
    for _ in range(3):
        x, idx, pos = pool5(x, policy)
        ys.append(x)
        idxs.append(idx)
        poss.append(pos)
    return ys, idxs, poss


def decode(pos):
    """position bytes [N, H, W, C] -> flat source indices"""
    N, H, W, C = pos.shape
    dy, dxp = (pos & 15).astype(np.int64), (pos >> 4).astype(np.int64)
    r = np.arange(H)[None, :, None, None] + dy - 2
    assert (dy <= 4).all() and (dxp <= 4).all() and (r >= 0).all() and (r < H).all(), 'a position byte points outside the plane'
    n, _, w, c = np.meshgrid(np.arange(N), np.arange(H), np.arange(W), np.arange(C), indexing='ij')
    col = w + dxp[n, r, w, c] - 2
    assert (col >= 0).all() and (col < W).all(), 'a position byte points outside the plane'
    return r * W + col


# ------------------------------------------------------------------------------------------ SPPF backward
def _scatter(t, idx):
    N, H, W, C = t.shape
    out = np.zeros((N, H * W, C), t.dtype)
    n, _, c = np.meshgrid(np.arange(N), np.arange(H * W), np.arange(C), indexing='ij')
    np.add.at(out, (n, idx.reshape(N, H * W, C), c), t.reshape(N, H * W, C))
    return out.reshape(N, H, W, C)


def sppf_bwd(gs, idxs, dtype=np.float64):
    """gs = (g0, g1, g2, g3), idxs = flat indices per level -> (dx, A); dtype=np.float32 gives the same expression rounded in fp32 (figures only)"""
    t, a = gs[3].astype(dtype), np.abs(gs[3].astype(dtype))
    for lv in (2, 1, 0):
        t = gs[lv].astype(dtype) + _scatter(t, idxs[lv])
        a = np.abs(gs[lv].astype(dtype)) + _scatter(a, idxs[lv])
    return t, a


def sppf_bwd_bound(A, bf16, ref):
    return finish(SPPF_ADDS * U * f64(A), ref, bf16)


# ------------------------------------------------------------------------------------------ upsample, layout
def upsample_fwd(x):
    return np.repeat(np.repeat(x, 2, axis=1), 2, axis=2)


def upsample_bwd(dy, old=None, dtype=np.float64):
    """-> (dx, A)"""
    N, H2, W2, C = dy.shape
    with np.errstate(all='ignore'):
        d = dy.reshape(N, H2 // 2, 2, W2 // 2, 2, C)
        s = np.zeros((N, H2 // 2, W2 // 2, C), dtype) if old is None else old.astype(dtype)
        a = np.abs(s)
        for i in range(2):
            for j in range(2):
                v = d[:, :, i, :, j, :].astype(dtype)
                s = s + v
                a = a + np.abs(v)
    return s, a


def upsample_bwd_bound(A, bf16, ref):
    return finish(UP_ADDS * U * f64(A), ref, bf16)


def stem_prep(img, pad, dt):
    B, _, H, W = img.shape
    out = np.zeros((B, H + 2 * pad, W + 2 * pad, 4), np.float32)
    out[:, pad:pad + H, pad:pad + W, :3] = np.transpose(img, (0, 2, 3, 1))
    return q(out, dt)


def nchw_to_nhwc(src, dt):
    return q(np.transpose(src, (0, 2, 3, 1)), dt)


# ------------------------------------------------------------------------------------------ bits
def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(got, want, nan_payload=True, zero_sign=True):
    """elementwise: equal bits; nan_payload=False: a NaN equals any NaN; zero_sign=False: +0 equals -0"""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    ok = bits(got) == bits(want)
    if not nan_payload:
        ok |= np.isnan(got) & np.isnan(want)
    if not zero_sign:
        ok |= (got == 0) & (want == 0)
    return ok
