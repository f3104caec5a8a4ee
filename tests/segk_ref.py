"""Float64 restatement of csrc/seg.hip (GroupNorm(+ReLU) forward / backward, the align-corners bilinear resize and its transpose, softmax +
soft-dice loss and gradient, the gradient followed by the W pass, softmax2d) in plain numpy: no autograd, no F.group_norm, no F.interpolate.
tests/test_segk_ref_host.py pins it to torch float64 autograd at 1e-12; tests/test_gpu_seg_direct.py compares the kernels with it.

Layouts: activations [N, HW, C] (GroupNorm) or [N, H, W, C] (resize), logits [N, HW, nc], targets [N, nc, HW].

The comparers (`ratios`, `check`) return the worst error in units of its bound and raise AssertionError above 1.  They exclude no
element and take no bound from a kernel's output: every bound below is computed from the reference and the launch geometry alone, from the
roundings the kernels perform (U = 2^-24 is one fp32 rounding; the library is built with -ffp-contract=off, so every fp32 product and sum
is rounded on its own).  The bounds are first order in U; SLACK = 1 + 2^-10 covers the second-order terms.

GroupNorm statistics (gn_reduce_kernel, gn_fwd_finalize_kernel).  A lane adds its pixels of one slice in fp32 (x*x by fma: one rounding
per step), the RL row lanes are added in fp32 through LDS, everything after that (32 slices, the channels of a group, mean, variance,
rstd) is double.  With n = trips + RL the longest fp32 chain, at most the number of pixels of a slice, since adding a lane that holds 0
is exact (segk_cases.gn_geometry):
    |dmean| <= n U E|x|
    |dvar|  <= (n + 1) U E[x^2] + 2 |mean| |dmean|              (var = E[x^2] - mean^2; the clamp at 0 is 1-Lipschitz)
The first term is the (n + c) 2^-24 E[x^2] of the sum of squares, c = 1 for the fma; the second is the error of the fp32 sum of x entering
through mean^2, a rounding the kernel really performs: at most 2n U E[x^2] more, and that much only where |mean| >> std (case 'offset':
drstd / rstd <= 0.20 with it, 0.09 from the first term alone; the table of test_gpu_seg_direct reports that group's measured error on its own).
    drstd / rstd <= dvar / (2 (var + eps))
so a group whose mean is 1000 times its spread is held to what E[x^2] - mean^2 from fp32 slice sums can deliver, no more and no less
(case 'offset': drstd / rstd <= 0.2; the measured error of that group is inside the bound, test_gpu_seg_direct's table).
stat = (mean, rstd) is cast to fp32 (U each).  Forward, a = fl(gamma rstd32), b = fl(beta - fl(mean32 a)), pre = fl(fl(x a) + b):
    |dpre| <= |xhat gamma| (drstd / rstd + 2U) + |a| |dmean| + U (3 |mean a| + |beta| + |x a| + |pre|)
(the error of `a` is common to x a and mean a, so it multiplies (x - mean) a = xhat gamma).  ReLU is 1-Lipschitz.

GroupNorm backward (from the forward's own stat / ab).  xhat32 = fl(fl(x - mean32) rstd32):
    |dxhat| <= |xhat| (drstd / rstd + 3U) + rstd (|dmean| + U |mean|)
A[n][c] = SUM dy and B[n][c] = SUM dy xhat32 go through the same chain n; the sums over slices, images and the group are double:
    |dA| <= n U SUM |dy|,    |dB| <= SUM ((n + 2) U |dy xhat| + |dy| |dxhat|)
    dbeta = SUM_n A, dgamma = SUM_n B: U |.| more for each cast (pc, the result), U (|old| + |sum|) when accumulated.
    k0 = fl(rstd32 gamma), k1 = rstd32 s1 / m, k2 = rstd32 s2 / m with s1 = SUM_c gamma A, s2 = SUM_c gamma B over the group:
    |dk1| <= |k1| (drstd / rstd + 2U) + rstd SUM |gamma| |dA| / m, k2 likewise from dB
    dx = fl(fl(fl(k0 dy) - k1) - fl(xhat32 k2)):
    |ddx| <= |k0 dy| (drstd / rstd + 2U) + |dk1| + |xhat| |dk2| + |k2| |dxhat| + U (3 |k0 dy| + 2 |k1| + 2 |xhat k2|)
a bound in the magnitudes of the three terms, not in |dx|: at HW == 1 with G == C, dx is exactly 0 and the kernel's k0 dy - k1 is not.

Resize.  scale32 = fl((in - 1) / (out - 1)) and s = fl(scale32 dst) are wrong by up to 2U s = 2^-23 s (one ulp of s or a little more);
l1 = s - i0 is exact, l0 = fl(1 - l1) adds U.  Moving weight ds between two neighbours changes the blend by ds |x[i1] - x[i0]|.  Only where s
is within ds of an integer can the fp32 index come out one lower or higher than i0 (case 'flip'); there, and only there, the larger of the
adjacent differences around i0 is taken, and the weight error is charged to the columns i0 - 1 .. i0 + 1 instead of (i0, i1).  The
four-term blend ly0 (wx0 a + wx1 b) + ly1 (wx0 c + wx1 d) is four roundings deep, two more for the l0s: 6U of the blend of |x|.
Transpose: dx[i] = SUM_o w(o, i) dy[o], added in fp32 in candidate order: (k + 3) U SUM |w dy| with k the number of contributing outputs,
plus SUM_o dw(o, i) |dy[o]| with dw = ds + U on the columns (i0, i1) of row o (the same term, on each contributing gradient).
Two passes: the W pass's result is rounded to the tensor's type before the H pass reads it.

Dice.  e = __expf(x) is v_exp_f32 on x log2(e): relative error <= (1 + |x|) 2^-23 for x = l - max (the guides' ISA notes give no other
figure), plus U |x| for the rounding of l - max itself; v_rcp_f32 adds 2^-23, the sum of nc terms (nc - 1) U, the product e inv U:
    dp / p <= eps_c + SUM_j p_j eps_j + (nc - 1) U + 2^-23 + U,    eps_c = (1 + |x_c|) 2^-23 + U |x_c|,    plus FLOOR = 2^-126 absolute
(an e below the smallest normal float is flushed to 0).  Slice sums: a lane's pixels, six shuffle steps, four waves in fp32
(n = trips + 10), slices in double:
    |dprod| <= SUM t dp + (n + 1) U SUM t p,    |dplus| <= SUM dp + (n + 1) U SUM (t + p)
    ddice = 2 dprod / plus + 2 prod dplus / plus^2;   dloss = SUM_c w_c mean_n ddice / SUM w + U |loss|
    ka = -2w / plus, kb = 2w prod / plus^2 (cast: U), q = fl(fl(ka t) + kb), dot = SUM q p, g = fl(fl(up p) fl(q - dot)):
    |dq| <= t |dka| + |dkb| + U (|ka t| + |q|);  |ddot| <= SUM (p |dq| + |q| dp) + (nc + 1) U SUM |q p|
    |dg| <= |up| (dp |q - dot| + p (|dq| + |ddot| + U |q - dot|)) + 2U |g|
softmax2d uses expf and an IEEE division, both within the figures above.

bf16 outputs: the kernel rounds its fp32 value once: 2^-8 (|ref| + bound) on top (half a bf16 ulp: 8 significand bits).
Bit equality of two kernel forms and the 1e-12 pin to torch float64 are the only other criteria in the new files.
"""
import numpy as np

U = 2.0 ** -24
ULP = 2.0 ** -23
FLOOR = 2.0 ** -126
SLACK = 1.0 + 2.0 ** -10
BF16_HALF_ULP = 2.0 ** -8
KINK_MARGIN = 64.0


def f64(a):
    return np.asarray(a, np.float64)


# ------------------------------------------------------------------------------------------ comparers
def finish(bound, ref, bf16, old=None):
    """the output stage on top of an fp32 bound: the accumulate (U (|old| + |ref|), `ref` being the total) and the bf16 rounding"""
    with np.errstate(all='ignore'):
        b = f64(bound) * SLACK
        if old is not None:
            b = b + U * (np.abs(f64(old)) + np.abs(f64(ref)))
        if bf16:
            b = b + BF16_HALF_ULP * (np.abs(f64(ref)) + b)
    return b


def ratios(got, ref, bound, what=''):
    """error / bound per element: NaN where and only where the reference has NaN, the same infinity where it has one (both asserted),
    |got - ref| / bound everywhere else"""
    got, ref, bound = f64(got), f64(ref), np.broadcast_to(f64(bound), np.shape(ref))
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), \
        f'{what}: NaN mask differs from the reference at {int((np.isnan(got) != np.isnan(ref)).sum())} of {ref.size} elements'
    inf = np.isinf(ref)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], ref[inf]), f'{what}: infinities differ from the reference'
    fin = np.isfinite(ref)
    err = np.abs(np.where(fin, got, 0.0) - np.where(fin, ref, 0.0))
    b = np.where(fin, bound, 1.0)
    assert np.isfinite(b).all() and (b >= 0).all(), f'{what}: the bound itself is not finite where the reference is'
    return np.where(err == 0, 0.0, err / np.maximum(b, 1e-300))


def check(got, ref, bound, what=''):
    """every element within its bound; returns the worst error / bound"""
    r = ratios(got, ref, bound, what)
    if r.size == 0:
        return 0.0
    k = np.unravel_index(int(np.argmax(r)), r.shape)
    assert r[k] <= 1.0, (f'{what}: element {k}: got {f64(got)[k]!r}, reference {f64(ref)[k]!r}: {r[k]:.3g} times the bound '
                         f'{np.broadcast_to(f64(bound), r.shape)[k]:.3g}')
    return float(r[k])


# ------------------------------------------------------------------------------------------ GroupNorm
def gn_stats(x, G):
    """two-pass (mean, var) per (image, group): [N, G] each"""
    x = f64(x)
    N, HW, C = x.shape
    with np.errstate(all='ignore'):
        xg = x.reshape(N, HW, G, C // G)
        mean = xg.mean((1, 3))
        var = ((xg - mean[:, None, :, None]) ** 2).mean((1, 3))
    return mean, var


def _per_channel(v, C):
    """[N, G] -> [N, 1, C]"""
    return np.repeat(v, C // v.shape[1], 1)[:, None, :]


def gn_forward(x, gamma, beta, G, eps, relu):
    """-> (y, pre): y = relu?(pre), pre = (x - mean) rstd gamma + beta; a ReLU that lets NaN through (F.relu)"""
    x, gamma, beta = f64(x), f64(gamma), f64(beta)
    C = x.shape[2]
    mean, var = gn_stats(x, G)
    with np.errstate(all='ignore'):
        rstd = 1.0 / np.sqrt(var + float(eps))
        pre = (x - _per_channel(mean, C)) * _per_channel(rstd, C) * gamma + beta
        y = np.where(pre < 0, 0.0, pre) if relu else pre
    return y, pre


def gn_backward(dout, x, gamma, beta, G, eps, relu):
    """-> (dx, dgamma, dbeta) of sum(dout * y); the ReLU gate from the forward pre-activation (0 where pre <= 0, dout elsewhere, NaN pre
    included: torch's threshold_backward)"""
    t = gn_terms(dout, x, gamma, beta, G, eps, relu)
    with np.errstate(all='ignore'):
        dx = t['k0'] * t['dy'] - t['k1'] - t['xhat'] * t['k2']
        return dx, (t['dy'] * t['xhat']).sum((0, 1)), t['dy'].sum((0, 1))


def gn_terms(dout, x, gamma, beta, G, eps, relu):
    dout, x, gamma = f64(dout), f64(x), f64(gamma)
    N, HW, C = x.shape
    m = HW * (C // G)
    mean, var = gn_stats(x, G)
    with np.errstate(all='ignore'):
        rstd = 1.0 / np.sqrt(var + float(eps))
        mc, rc = _per_channel(mean, C), _per_channel(rstd, C)
        xhat = (x - mc) * rc
        pre = xhat * gamma + f64(beta)
        dy = np.where(pre <= 0, 0.0, dout) if relu else dout
        gsum = lambda a: _per_channel(a.reshape(N, HW, G, C // G).sum((1, 3)), C)           # noqa: E731
        k0 = rc * gamma
        k1 = rc * gsum(gamma * dy) / m
        k2 = rc * gsum(gamma * dy * xhat) / m
    return dict(dy=dy, xhat=xhat, pre=pre, k0=k0, k1=k1, k2=k2, mean=mc, rstd=rc, var=_per_channel(var, C), m=m)


def gn_stat_errors(x, G, eps, n):
    """(|dmean|, drstd / rstd) per (image, group) as [N, 1, C], from the chain length n"""
    x = f64(x)
    N, HW, C = x.shape
    mean, var = gn_stats(x, G)
    with np.errstate(all='ignore'):
        xg = x.reshape(N, HW, G, C // G)
        e1, e2 = np.abs(xg).mean((1, 3)), (xg * xg).mean((1, 3))
        dmean = n * U * e1
        dvar = (n + 1) * U * e2 + 2 * np.abs(mean) * dmean
        drel = dvar / (2 * (var + float(eps)))
    return _per_channel(dmean, C), _per_channel(drel, C)


def gn_forward_bound(x, gamma, beta, G, eps, n):
    """fp32 bound of the pre-activation (and of the ReLU output) per element; not finite only where the reference is not"""
    x, gamma, beta = f64(x), f64(gamma), f64(beta)
    C = x.shape[2]
    mean, var = gn_stats(x, G)
    dmean, drel = gn_stat_errors(x, G, eps, n)
    with np.errstate(all='ignore'):
        mc = _per_channel(mean, C)
        rc = _per_channel(1.0 / np.sqrt(var + float(eps)), C)
        a = rc * gamma
        pre = (x - mc) * a + beta
        return (np.abs((x - mc) * a) * (drel + 2 * U) + np.abs(a) * dmean
                + U * (3 * np.abs(mc * a) + np.abs(beta) + np.abs(x * a) + np.abs(pre)))


def gn_backward_bounds(dout, x, gamma, beta, G, eps, relu, n):
    """fp32 bounds (dx [N, HW, C], dgamma [C], dbeta [C]) before the casts of the parameter gradients (see gn_param_bound)"""
    t = gn_terms(dout, x, gamma, beta, G, eps, relu)
    gamma = f64(gamma)
    N, HW, C = np.shape(x)
    dmean, drel = gn_stat_errors(x, G, eps, n)
    with np.errstate(all='ignore'):
        dy, xhat, rstd = np.abs(t['dy']), np.abs(t['xhat']), t['rstd']
        dxhat = xhat * (drel + 3 * U) + rstd * (dmean + U * np.abs(t['mean']))
        dA = (n * U * dy).sum(1, keepdims=True)                                               # [N, 1, C]
        dB = ((n + 2) * U * dy * xhat + dy * dxhat).sum(1, keepdims=True)
        gsum = lambda a: _per_channel(a.reshape(N, 1, G, C // G).sum((1, 3)), C)             # noqa: E731
        dk1 = np.abs(t['k1']) * (drel + 2 * U) + rstd * gsum(np.abs(gamma) * dA) / t['m']
        dk2 = np.abs(t['k2']) * (drel + 2 * U) + rstd * gsum(np.abs(gamma) * dB) / t['m']
        a0, a1, a2 = np.abs(t['k0'] * t['dy']), np.abs(t['k1']), np.abs(t['xhat'] * t['k2'])
        bdx = a0 * (drel + 2 * U) + dk1 + xhat * dk2 + np.abs(t['k2']) * dxhat + U * (3 * a0 + 2 * a1 + 2 * a2)
        A, B = np.abs(t['dy'].sum(1, keepdims=True)), np.abs((t['dy'] * t['xhat']).sum(1, keepdims=True))
        bdb = (dA + U * A).sum((0, 1))                                                        # + the cast of pc per image
        bdg = (dB + U * B).sum((0, 1))
    return bdx, bdg, bdb


def gn_param_bound(b, total, old=None):
    """the final cast of a parameter gradient, and the fp32 add when it is accumulated into `old` (`total` includes `old`)"""
    with np.errstate(all='ignore'):
        t, o = np.abs(f64(total)), (np.abs(f64(old)) if old is not None else 0.0)
        return SLACK * f64(b) + U * (t + o) + (U * (t + o) if old is not None else 0.0)


# ------------------------------------------------------------------------------------------ resize
def resize_axis(n_in, n_out):
    """align_corners weights of one axis: (R [out, in], dR [out, in] the bound of every weight's error, s [out], i0 [out], near [out]).
    near[o]: s is within its own error 2^-23 s of an integer, so the fp32 index may come out one lower or higher than i0; only there does the
    weight error reach the columns i0 - 1 .. i0 + 1, everywhere else it stays on (i0, i1)."""
    scale = (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0
    R, dR = np.zeros((n_out, n_in)), np.zeros((n_out, n_in))
    s = scale * np.arange(n_out)
    i0 = np.minimum(np.floor(s).astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = s - i0
    near = (s > 0) & (np.abs(s - np.rint(s)) <= ULP * s)
    for o in range(n_out):
        R[o, i0[o]] += 1.0 - l1[o]
        R[o, i1[o]] += l1[o]
        lo, hi = (max(i0[o] - 1, 0), min(i0[o] + 1, n_in - 1)) if near[o] else (i0[o], i1[o])
        dR[o, lo:hi + 1] = ULP * s[o] + U
    return R, dR, s, i0, near


def _adjacent(a, axis, i0, near):
    """|a[i1] - a[i0]| along `axis` per output index o; where near[o], the largest of that and of the pairs before and after it"""
    a = np.moveaxis(f64(a), axis, 0)
    d = np.abs(np.diff(a, axis=0))
    z = np.zeros((1,) + a.shape[1:])
    left, right = np.concatenate([z, d]), np.concatenate([d, z])        # |a[i] - a[i-1]|, |a[i+1] - a[i]|
    wide = np.maximum(np.maximum(left, right), np.concatenate([right[1:], z]))
    sel = near.reshape((-1,) + (1,) * (a.ndim - 1))
    return np.moveaxis(np.where(sel, wide[i0], right[i0]), 0, axis)


def resize_forward(x, size):
    """x [N, Hi, Wi, C] -> (y [N, Ho, Wo, C], fp32 bound)"""
    x = f64(x)
    Ry, _, sy, y0, ny = resize_axis(x.shape[1], size[0])
    Rx, _, sx, x0, nx = resize_axis(x.shape[2], size[1])
    xw = np.einsum('nhwc,ow->nhoc', x, Rx)
    y = np.einsum('nhoc,ph->npoc', xw, Ry)
    xh = np.einsum('nhwc,ph->npwc', x, Ry)
    mag = np.einsum('nhwc,ow,ph->npoc', np.abs(x), Rx, Ry)
    by = (ULP * sy + U)[None, :, None, None] * _adjacent(xw, 1, y0, ny)
    bx = (ULP * sx + U)[None, None, :, None] * _adjacent(xh, 2, x0, nx)
    return y, 6 * U * mag + by + bx


def _axis_T(g, R, axis):
    return np.einsum('nhwc,hi->niwc' if axis == 1 else 'nhwc,wi->nhic', g, R)


def _terms(R, dR):
    """[in]: how many outputs can contribute to an input (k of the summation bound)"""
    return ((R != 0) | (dR != 0)).sum(0)


def resize_backward(dy, in_size):
    """the transpose: dy [N, Ho, Wo, C] -> dx [N, Hi, Wi, C]"""
    dy = f64(dy)
    Ry = resize_axis(in_size[0], dy.shape[1])[0]
    Rx = resize_axis(in_size[1], dy.shape[2])[0]
    return _axis_T(_axis_T(dy, Rx, 2), Ry, 1)


def resize_backward_axis(dy, n_in, axis, bin_=None):
    """one axis of the transpose -> (dx, fp32 bound); bin_: the error bound `dy` already carries"""
    dy = f64(dy)
    R, dR = resize_axis(n_in, dy.shape[axis])[:2]
    k = _terms(R, dR).reshape((1, -1, 1, 1) if axis == 1 else (1, 1, -1, 1))
    a = np.abs(dy)
    b = (k + 3) * U * _axis_T(a, R, axis) + _axis_T(a, dR, axis)
    if bin_ is not None:
        b = b + _axis_T(f64(bin_), R + dR, axis)
    return _axis_T(dy, R, axis), b


def resize_backward_bound(dy, in_size, form, bf16):
    """fp32 bound of the transpose as `form` computes it: '2d' (one gather, weights fl(wy wx)) or 'two-pass' (W pass, its result rounded to
    the tensor's type, then the H pass)"""
    dy = f64(dy)
    a = np.abs(dy)
    Ry, dRy = resize_axis(in_size[0], dy.shape[1])[:2]
    Rx, dRx = resize_axis(in_size[1], dy.shape[2])[:2]
    if form == '2d':
        k = _terms(Ry, dRy)[None, :, None, None] * _terms(Rx, dRx)[None, None, :, None]
        T = lambda gy, gx: _axis_T(_axis_T(a, gx, 2), gy, 1)                                  # noqa: E731
        return (k + 4) * U * T(Ry, Rx) + T(dRy, Rx) + T(Ry, dRx) + T(dRy, dRx)
    assert form == 'two-pass'
    tmp, bw = resize_backward_axis(dy, in_size[1], 2)
    bw = finish(bw, tmp, bf16)
    return resize_backward_axis(tmp, in_size[0], 1, bw)[1]


# ------------------------------------------------------------------------------------------ softmax, soft dice
def softmax(l):
    """over the last axis; NaN for every class of a pixel that holds a NaN"""
    l = f64(l)
    with np.errstate(all='ignore'):
        e = np.exp(l - l.max(-1, keepdims=True))
        return e / e.sum(-1, keepdims=True)


def softmax_error(l):
    """absolute bound of a probability (module docstring)"""
    l = f64(l)
    nc = l.shape[-1]
    with np.errstate(all='ignore'):
        x = np.abs(l - l.max(-1, keepdims=True))
        p = softmax(l)
        eps = (1 + x) * ULP + U * x
        return p * (eps + (p * eps).sum(-1, keepdims=True) + (nc - 1) * U + ULP + U) + FLOOR


def dice_parts(logits, targets, weights):
    l, t = f64(logits), np.moveaxis(f64(targets), 1, 2)                   # t [N, HW, nc]
    N, HW, nc = l.shape
    w = np.ones(nc) if weights is None else f64(weights)
    p = softmax(l)
    with np.errstate(all='ignore'):
        prod, plus = (t * p).sum(1), (t + p).sum(1)                        # [N, nc]
        dice = 2 * prod / plus
        loss = 1.0 - (w * dice.mean(0)).sum() / w.sum()
    return dict(l=l, t=t, p=p, w=w / (w.sum() * N), prod=prod, plus=plus, dice=dice, loss=loss)


def dice_loss(logits, targets, weights=None):
    return dice_parts(logits, targets, weights)['loss']


def dice_grad(logits, targets, weights=None, upstream=1.0):
    """d (upstream loss) / d logits [N, HW, nc]: d loss / d p = -w (2 t / plus - 2 prod / plus^2), then the softmax Jacobian"""
    d = dice_parts(logits, targets, weights)
    with np.errstate(all='ignore'):
        q = -d['w'] * (2 * d['t'] / d['plus'][:, None] - 2 * d['prod'][:, None] / d['plus'][:, None] ** 2)
        return float(upstream) * d['p'] * (q - (q * d['p']).sum(-1, keepdims=True))


def dice_bounds(logits, targets, weights, upstream, n):
    """(bound of the loss, bound of the gradient [N, HW, nc]); n: the fp32 chain of a slice sum (segk_cases.dice_chain)"""
    d = dice_parts(logits, targets, weights)
    t, p, w, prod, plus = np.abs(d['t']), d['p'], d['w'], d['prod'], d['plus']
    nc = p.shape[-1]
    up = abs(float(upstream))
    with np.errstate(all='ignore'):
        dp = softmax_error(d['l'])
        dprod = (t * dp).sum(1) + (n + 1) * U * (t * p).sum(1)
        dplus = dp.sum(1) + (n + 1) * U * (t + p).sum(1)
        ddice = 2 * dprod / plus + 2 * np.abs(prod) * dplus / plus ** 2
        bloss = SLACK * (w * ddice).sum() + U * abs(d['loss'])
        ka, kb = -2 * w / plus, 2 * w * prod / plus ** 2
        dka = np.abs(ka) * (dplus / plus + U)
        dkb = 2 * w * (dprod / plus ** 2 + 2 * np.abs(prod) * dplus / plus ** 3) + U * np.abs(kb)
        q = ka[:, None] * d['t'] + kb[:, None]
        dq = t * dka[:, None] + dkb[:, None] + U * (np.abs(ka[:, None] * d['t']) + np.abs(q))
        dot = (q * p).sum(-1, keepdims=True)
        ddot = (p * dq + np.abs(q) * dp).sum(-1, keepdims=True) + (nc + 1) * U * np.abs(q * p).sum(-1, keepdims=True)
        g = up * p * (q - dot)
        bg = up * (dp * np.abs(q - dot) + p * (dq + ddot + U * np.abs(q - dot))) + 2 * U * np.abs(g)
    return bloss, SLACK * bg
