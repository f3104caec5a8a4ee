"""Float64 restatement of csrc/bn_act.hip (BatchNorm finalize, activation forward, backward, column sums, eval coefficients, the
SyncBatchNorm algebra) in plain numpy: no autograd, no F.batch_norm.  tests/test_bn_ref_host.py pins it to torch float64 autograd;
tests/test_gpu_bn_direct.py compares the kernels with it.  Tensors are [M, K] arrays (rows x channels), per-channel vectors are [K].

Every stage takes its inputs as given (the fp32 slabs, the fp32 scale / shift / mean / invstd) and evaluates them in float64, so a stage is
judged on its own arithmetic and inherits no rounding of the stage before it.

The comparers (`check_*`) return the worst error in units of its bound and raise AssertionError above 1.  Every bound is derived from the
roundings the kernel performs (u = 2^-24 is one fp32 rounding, ulp = 2^-23 = 2u); none comes from a kernel's output.  The library is
built with -ffp-contract=off, so every fp32 product and sum below is rounded on its own.
"""
import numpy as np

U32 = 2.0 ** -24
ULP = 2.0 ** -23
ACT_NONE, ACT_SILU, ACT_RELU = 0, 1, 2
RTOL32, ATOL32_RMS = 1e-4, 0.2e-4            # the project's fp32 criterion (assert_close of tests/test_gpu_kernels.py)
FINALIZE_ULPS = {'mean': 1, 'invstd': 1, 'scale': 2, 'shift': 3, 'rm': 2, 'rv': 2}
FINALIZE_NAMES = ('scale', 'shift', 'mean', 'invstd', 'rm', 'rv')


def f64(a):
    return np.asarray(a, np.float64)


# ------------------------------------------------------------------------------------------ activations
def act_fwd(u, act):
    """SiLU as u / (1 + exp(-u)) (NaN at -inf, like the kernel's u * rcp(1 + exp(-u))); ReLU as a select that lets NaN through (F.relu)"""
    with np.errstate(all='ignore'):
        if act == ACT_SILU:
            return u / (1.0 + np.exp(-u))
        if act == ACT_RELU:
            return np.where(u < 0, 0.0, u)
    return u


def act_grad(u, act):
    assert act in (ACT_NONE, ACT_SILU), 'the BatchNorm backward exists for no activation and SiLU'
    if act == ACT_NONE:
        return np.ones_like(u)
    with np.errstate(over='ignore'):
        s = 1.0 / (1.0 + np.exp(-u))
    return s * (1.0 + u * (1.0 - s))


# ------------------------------------------------------------------------------------------ finalize
def finalize_from_sums(s, ss, count, gamma, beta, rm, rv, eps, momentum):
    """(scale, shift, mean, invstd, rm', rv') from per-channel SUM and SUM of squares: biased variance clamped at 0 for the normalisation,
    unbiased for the running value except at count == 1 where it stays biased.  rm / rv None: no running statistics (rm' = rv' = None)."""
    s, ss, gamma, beta, count = f64(s), f64(ss), f64(gamma), f64(beta), float(count)
    mean = s / count
    var = np.maximum(ss / count - mean * mean, 0.0)
    invstd = 1.0 / np.sqrt(var + float(eps))
    scale = gamma * invstd
    shift = beta - mean * scale
    if rm is None:
        return scale, shift, mean, invstd, None, None
    unbiased = var * count / (count - 1.0) if count > 1 else var
    m = float(momentum)
    return scale, shift, mean, invstd, (1.0 - m) * f64(rm) + m * mean, (1.0 - m) * f64(rv) + m * unbiased


def finalize(slabs, count, gamma, beta, rm, rv, eps, momentum):
    """slabs [n][2][K]: the fp32 per-tile (SUM, SUM of squares) as given, added in float64"""
    t = f64(slabs).sum(0)
    return finalize_from_sums(t[0], t[1], count, gamma, beta, rm, rv, eps, momentum)


def finalize_bounds(slabs, count, gamma, beta, rm, rv, eps, momentum):
    """Per-channel bounds for the six finalize outputs, FINALIZE_ULPS[name] ulps of the largest term plus a float64 term.

    The kernel adds the slabs in float64 in another order and forms mean and var in float64: with E = 2^-40 * SUM|slab| (n <= 8192 slabs at
    2^-53 each), dmean = E_s / count, dvar = E_ss / count + 2 |mean| dmean + 2^-50 (ss / count + mean^2), dinvstd = invstd^3 dvar / 2 (the
    clamp at 0 is 1-Lipschitz, so it changes nothing).  These terms are 2^-16 of an ulp unless mean^2 >> var.  Then, in fp32:
      mean, invstd   one cast each: u <= 1 ulp of itself.
      scale          fl(gamma * invstd32): the cast and the product, 2u = 1 ulp; bound 2 ulps of |scale|.
      shift          fl(beta - fl(mean32 * scale32)): mean's cast u, scale's 2u, the product u on |mean * scale|, the subtraction u on
                     |shift| <= |beta| + |mean * scale|: 5u = 2.5 ulps; bound 3 ulps of |beta| + |mean * scale|.
      rm', rv'       fl(fl(fl(1 - m) * old) + fl(m * new32)): fl(1 - m) and the product put 2u on |(1 - m) old|, the cast and the product 2u on
                     |m new|, the sum u on both: 3u = 1.5 ulps; bound 2 ulps of |(1 - m) old| + |m new|.
    """
    a = np.abs(f64(slabs)).sum(0)
    scale, shift, mean, invstd, rm1, rv1 = finalize(slabs, count, gamma, beta, rm, rv, eps, momentum)
    t = f64(slabs).sum(0)
    count, m = float(count), float(momentum)
    dmean = 2.0 ** -40 * a[0] / count
    dvar = 2.0 ** -40 * a[1] / count + 2 * np.abs(mean) * dmean + 2.0 ** -50 * (t[1] / count + mean * mean)
    dinv = 0.5 * invstd ** 3 * dvar
    g = np.abs(f64(gamma))
    k = FINALIZE_ULPS
    out = {'mean': k['mean'] * ULP * np.abs(mean) + dmean,
           'invstd': k['invstd'] * ULP * invstd + dinv,
           'scale': k['scale'] * ULP * np.abs(scale) + g * dinv,
           'shift': k['shift'] * ULP * (np.abs(f64(beta)) + np.abs(mean * scale)) + np.abs(scale) * dmean + np.abs(mean) * g * dinv}
    if rm is not None:
        var = np.maximum(t[1] / count - mean * mean, 0.0)
        unb = var * count / (count - 1.0) if count > 1 else var
        out['rm'] = k['rm'] * ULP * (np.abs((1 - m) * f64(rm)) + np.abs(m * mean)) + m * dmean
        out['rv'] = k['rv'] * ULP * (np.abs((1 - m) * f64(rv)) + np.abs(m * unb)) + m * dvar * (count / (count - 1.0) if count > 1 else 1.0)
    return out


def check_vector(got, ref, bound, what=''):
    """|got - ref| <= bound for every channel; returns the worst error / bound"""
    got, ref, bound = f64(got), f64(ref), f64(bound)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), f'{what}: not finite'
    err = np.abs(got - ref)
    ratio = np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))
    k = int(np.argmax(ratio))
    assert ratio.flat[k] <= 1.0, f'{what}: channel {k}: got {got.flat[k]!r}, reference {ref.flat[k]!r}: {ratio.flat[k]:.3g} times the bound {bound.flat[k]:.3g}'
    return float(ratio.flat[k])


def check_finalize(got, ref, bounds, what=''):
    """got / ref: (scale, shift, mean, invstd, rm', rv'), rm' / rv' None where the module keeps no running statistics"""
    worst = 0.0
    for name, g, r in zip(FINALIZE_NAMES, got, ref):
        if r is None:
            assert g is None, name
            continue
        worst = max(worst, check_vector(g, r, bounds[name], f'{what} {name}'))
    return worst


# ------------------------------------------------------------------------------------------ forward
def forward(y, scale, shift, act, res=None):
    with np.errstate(invalid='ignore'):
        z = act_fwd(f64(y) * f64(scale) + f64(shift), act)
        return z if res is None else z + f64(res)


def elementwise_bound(ref, bf16):
    """fp32 outputs: the project's criterion, |err| <= 1e-4 |ref| + 0.2e-4 rms(ref) for EVERY element (rms over the finite elements).
    bf16 outputs: the kernel computes in fp32 from the same operands and rounds once, so 2^-8 |ref| (half a bf16 ulp: 8 significand bits)
    comes on top.  No element is excluded: at the ReLU kink |u| is inside the bound already."""
    ref = f64(ref)
    fin = np.isfinite(ref)
    rms = float(np.sqrt(np.mean(ref[fin] ** 2))) if fin.any() else 0.0
    a = np.abs(np.where(fin, ref, 0.0))
    return RTOL32 * a + ATOL32_RMS * rms + (2.0 ** -8 * a if bf16 else 0.0)


def check_elementwise(got, ref, bf16, what=''):
    """NaN where and only where the reference has NaN, the same infinity where it has one, elementwise_bound() everywhere else"""
    got, ref = f64(got), f64(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), \
        f'{what}: NaN mask differs from the reference at {int((np.isnan(got) != np.isnan(ref)).sum())} elements'
    inf = np.isinf(ref)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], ref[inf]), f'{what}: infinities differ from the reference'
    fin = np.isfinite(ref)
    err = np.abs(np.where(fin, got, 0.0) - np.where(fin, ref, 0.0))
    bound = elementwise_bound(ref, bf16)
    ratio = np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))
    k = np.unravel_index(int(np.argmax(ratio)), ratio.shape) if ratio.size else ()
    worst = float(ratio[k]) if ratio.size else 0.0
    assert worst <= 1.0, f'{what}: element {k}: got {got[k]!r}, reference {ref[k]!r}: {worst:.3g} times the bound {bound[k]:.3g}'
    return worst


# ------------------------------------------------------------------------------------------ backward
def backward_terms(dz, y, scale, shift, mean, invstd, act):
    """(du, xhat): du = dz * act'(y * scale + shift), xhat = (y - mean) * invstd"""
    dz, y = f64(dz), f64(y)
    du = dz * act_grad(y * f64(scale) + f64(shift), act)
    return du, (y - f64(mean)) * f64(invstd)


def backward(dz, y, scale, shift, mean, invstd, act, count):
    """(du, dbeta, dgamma, c1, c2, dy) of z = act(BN_train(y)): dbeta = SUM du, dgamma = SUM du * xhat, c1 = dbeta / count,
    c2 = dgamma / count, dy = scale * (du - c1 - xhat * c2).  `count` differs from the number of rows only under SyncBatchNorm."""
    du, xhat = backward_terms(dz, y, scale, shift, mean, invstd, act)
    dbeta, dgamma = du.sum(0), (du * xhat).sum(0)
    c1, c2 = dbeta / float(count), dgamma / float(count)
    return du, dbeta, dgamma, c1, c2, f64(scale) * (du - c1 - xhat * c2)


def backward_abs_sums(dz, y, scale, shift, mean, invstd, act):
    """(SUM |du|, SUM |du * xhat|) per channel: what the summation bound scales with"""
    du, xhat = backward_terms(dz, y, scale, shift, mean, invstd, act)
    return np.abs(du).sum(0), np.abs(du * xhat).sum(0)


def backward_frozen(dz, y, scale, shift, act):
    """frozen BatchNorm (constant scale / shift): dy = scale * dz * act'(u)"""
    return f64(scale) * f64(dz) * act_grad(f64(y) * f64(scale) + f64(shift), act)


def colsum(dz):
    """(SUM, SUM | |) over the rows"""
    dz = f64(dz)
    return dz.sum(0), np.abs(dz).sum(0)


def slab_finalize(slabs, count, mean, invstd):
    """slabs [n][2][K] of (SUM du, SUM du * y) from a producer's epilogue -> (dbeta, dgamma = invstd * (S2 - mean * S1), c1, c2) and the
    bounds of dbeta / dgamma: the sums are float64 on both sides (2^-40 SUM|slab| covers another order), the result is cast once (u)."""
    t, a = f64(slabs).sum(0), np.abs(f64(slabs)).sum(0)
    mean, invstd = f64(mean), f64(invstd)
    dbeta, dgamma = t[0], invstd * (t[1] - mean * t[0])
    bb = U32 * np.abs(dbeta) + 2.0 ** -40 * a[0]
    bg = U32 * np.abs(dgamma) + 2.0 ** -40 * invstd * (a[1] + np.abs(mean) * a[0])
    return dbeta, dgamma, dbeta / float(count), dgamma / float(count), bb, bg


def yardstick_c(dz, y, scale, shift, mean, invstd, act):
    """`c` of sum_bound(): what the evaluation of one term costs, in fp32 roundings.  dsilu_f uses the hardware exp and reciprocal, whose
    error cannot be derived here, so the yardstick is the same formulas in plain float32 (numpy exp and division), xhat in both forms the
    kernels use ((y - mean) * invstd and y * invstd + (-mean * invstd)): per channel, SUM_m |term32_m - term64_m| / SUM_m |term64_m|, the worst
    of the channels, of the two sums and of the two forms, times four, in units of 2^-24; plus 1 for the cast of the finished sum to fp32.
    (The error is taken term by term, before any cancellation between terms, and set against the same SUM |term| the bound multiplies.)"""
    f = np.float32
    dz32, y32, sc, sh, mu, inv = (np.asarray(a, f) for a in (dz, y, scale, shift, mean, invstd))
    du64, xh64 = backward_terms(dz, y, scale, shift, mean, invstd, act)
    u = y32 * sc + sh
    if act == ACT_SILU:
        with np.errstate(over='ignore'):
            s = f(1) / (f(1) + np.exp(-u))
        du32 = dz32 * (s * (f(1) + u * (f(1) - s)))
    else:
        du32 = dz32
    worst = 0.0
    for xh32 in ((y32 - mu) * inv, y32 * inv + (-mu * inv)):
        for t32, t64 in ((du32, du64), (du32 * xh32, du64 * xh64)):
            assert t32.dtype == f
            den = np.abs(t64).sum(0)
            num = np.abs(f64(t32) - t64).sum(0)
            worst = max(worst, float(np.max(np.where(den > 0, num / np.maximum(den, 1e-300), 0.0))))
    return 4.0 * worst / U32 + 1.0


def sum_bound(abs_sum, n, c, extra=0.0):
    """Worst-case fp32 summation bound (n + c) * 2^-24 * SUM_m |term_m|: n is the longest fp32 chain a value goes through (a lane's rows, then
    the workgroup's RL row lanes; slab-to-slab accumulation is float64 and adds nothing), c the cost of a term (yardstick_c; 1 where the
    terms are exact).  `extra`: u * (|old| + |sum|) where the result is added to an fp32 gradient already there."""
    return (n + c) * U32 * f64(abs_sum) + extra


# ------------------------------------------------------------------------------------------ eval coefficients, SyncBatchNorm
def eval_coeffs(gamma, beta, rm, rv, eps):
    scale = f64(gamma) / np.sqrt(f64(rv) + float(eps))
    return scale, f64(beta) - f64(rm) * scale


def eval_bounds(gamma, beta, rm, rv, eps):
    """scale = fl(gamma / sqrtf(fl(rv + eps))): the sum u / 2 after the root, the root and the division one ulp at most each: 3 ulps of
    |scale|.  shift = fl(beta - fl(rm * scale)): 3 ulps from scale and u from the product on |rm * scale|, u from the subtraction: 4 ulps
    of |beta| + |rm * scale|."""
    scale, _ = eval_coeffs(gamma, beta, rm, rv, eps)
    return 3 * ULP * np.abs(scale), 4 * ULP * (np.abs(f64(beta)) + np.abs(f64(rm) * scale))


def sync_sums(slab_sets, counts):
    """SyncBatchNorm: every rank's slabs summed to [SUM | SUM2 | count] (2K + 1 doubles), the ranks' blocks added together"""
    K = slab_sets[0].shape[2]
    total = np.zeros(2 * K + 1)
    for slabs, count in zip(slab_sets, counts):
        t = f64(slabs).sum(0)
        total += np.concatenate([t[0], t[1], [float(count)]])
    return total


def sync_coeffs(sums):
    """c1, c2 from the global [SUM du | SUM du * xhat | count]"""
    K = (len(sums) - 1) // 2
    return sums[:K] / sums[2 * K], sums[K:2 * K] / sums[2 * K]
