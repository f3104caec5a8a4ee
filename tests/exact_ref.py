"""Integer operands, a float64 CPU reference and a bitwise comparer for the convolution kernels (plain torch, no GPU).

With small integer operands every product and every partial sum of a convolution is exactly representable — in an fp32 accumulator, in
the fp32 MFMA path and in a bf16 output up to |v| <= 256 — so the result does not depend on the summation order, the split count, the
tile order or the kernel family, and the test of a kernel becomes equality with a float64 convolution on the CPU.  One wrong, missing or
doubled product term anywhere in the tensor fails it, and so does one pixel too many or too few in a BatchNorm statistics slab.

Operands of a case (N, H, W, C, K, R, stride, pad) — or, with a rectangular window, (N, H, W, C, K, R, S, stride, pad) — all from seeded generators:

    x        integers in [-2, 2]                     dy       integers in [-1, 1]
    w        +-1 with probability pw, else 0:        pw = min(1, V / (2 T)),  T = max(C, K) R S,  V = min(300, 8e6 / M),  M = N Ho Wo
    scale    cycles through 0.5, 1, 2, -1            shift    integers in [-8, 8]
    res, acc integers in [-4, 4]  (the residual operand and what an accumulating call finds in its output)
    stem     (6x6 / stride 2 / pad 2 over 3 channels) image values are integers in [0, 2] and T = 108

V is the variance budget of one output (each non-zero weight adds E[x^2] = 2): it keeps |y| small enough for bf16 and the per-channel
sum of squares below 2^24.  The sparse filters do not hide a misread: a wrong x element meets a non-zero weight in some filter with
probability 1 - (1 - pw)^K, and x and dy are dense, so a wrong weight element always shows.

The preconditions that make the comparison exact are asserted on the reference itself (`check_preconditions`); a case that violates one
is an error in the test's design and fails loudly — it is never skipped.
"""
import functools

import torch
import torch.nn.functional as F

SCALES = (0.5, 1.0, 2.0, -1.0)
Y_MAX = 122            # 2 |y| + 8 + 4 <= 256: the scaled, shifted and accumulated output is exact in bf16 (half-integers from scale 0.5 stay below 128)
DX_MAX = 252           # |dx| + 4 <= 256
SUM_MAX = 2 ** 24      # integers an fp32 sum holds exactly

AXES_NHWC = ('n', 'y', 'x', 'channel')
AXES_W = ('k', 'c', 'r', 's')
AXES_STAT = ('slab', 'stat', 'k')


def out_dim(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def ints(shape, lo, hi, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def window(case):
    """(N, H, W, C, K, R, S, stride, pad) of a case given with a square window (8 numbers) or a rectangular one (9)"""
    if len(case) == 9:
        return tuple(case)
    N, H, W, C, K, R, stride, pad = case
    return (N, H, W, C, K, R, R, stride, pad)


def weight_density(case, stem=False):
    N, H, W, C, K, R, S, stride, pad = window(case)
    M = N * out_dim(H, R, stride, pad) * out_dim(W, S, stride, pad)
    T = 108 if stem else max(C, K) * R * S
    V = min(300.0, 8.0e6 / M)
    return min(1.0, V / (2.0 * T))


def stem_case(N, H, W, K):
    return (N, H, W, 3, K, 6, 2, 2)


class Exact:
    """operands and float64 reference results of one case, all NCHW on the CPU"""


@functools.lru_cache(maxsize=2)
def reference(case, stem=False):
    """Operands and everything the legs compare against, computed once per case (the cache holds the last two cases: tests that share a
    case run back to back).  Nothing in it may be modified by a test."""
    N, H, W, C, K, R, S, stride, pad = window(case)
    Ho, Wo = out_dim(H, R, stride, pad), out_dim(W, S, stride, pad)
    e = Exact()
    e.case, e.stem, e.Ho, e.Wo, e.M = case, stem, Ho, Wo, N * Ho * Wo
    e.pw = weight_density(case, stem)
    e.x = ints((N, C, H, W), 0, 2, 1) if stem else ints((N, C, H, W), -2, 2, 1)
    g = torch.Generator().manual_seed(2)
    keep = (torch.rand((K, C, R, S), generator=g) < e.pw).double()
    e.w = (ints((K, C, R, S), 0, 1, 3) * 2 - 1) * keep
    e.dy = ints((N, K, Ho, Wo), -1, 1, 5)
    e.scale = torch.tensor([SCALES[k % 4] for k in range(K)], dtype=torch.float64)
    e.shift = ints((K,), -8, 8, 6)
    e.res = ints((N, K, Ho, Wo), -4, 4, 7)
    e.acc = ints((N, K, Ho, Wo), -4, 4, 8)
    e.dx_acc = ints((N, C, H, W), -4, 4, 9)
    xr, wr = e.x.clone().requires_grad_(True), e.w.clone().requires_grad_(True)
    y = F.conv2d(xr, wr, None, stride, pad)
    y.backward(e.dy)
    e.y, e.dx, e.dw = y.detach(), xr.grad, wr.grad
    e.sum, e.sumsq = e.y.sum((0, 2, 3)), (e.y * e.y).sum((0, 2, 3))
    e.affine = e.y * e.scale.view(1, -1, 1, 1) + e.shift.view(1, -1, 1, 1)          # the epilogue's scale * conv + shift, exact
    return e


def check_preconditions(e):
    """The conditions under which every leg of the case is exact, on the reference alone.  They are not skips."""
    ymax, dxmax = e.y.abs().max().item(), e.dx.abs().max().item()
    assert ymax <= Y_MAX, f'{e.case}: max |y| = {ymax} > {Y_MAX}: the epilogue legs would round in bf16'
    # the stem has no data gradient (its input is the image), so no leg ever holds dx and its bound does not apply there
    assert e.stem or dxmax <= DX_MAX, f'{e.case}: max |dx| = {dxmax} > {DX_MAX}: the accumulated data gradient would round in bf16'
    assert e.sumsq.max().item() < SUM_MAX, f'{e.case}: a channel has SUM y^2 = {e.sumsq.max().item():.0f} >= 2^24: fp32 partial sums would round'
    zero = (e.w.abs().sum((1, 2, 3)) == 0).nonzero().flatten().tolist()
    assert not zero, f'{e.case}: filters {zero} are all zero'
    assert e.dw.abs().max().item() < SUM_MAX, f'{e.case}: a weight gradient reaches 2^24'
    for t in (e.y, e.dx, e.dw, e.sum, e.sumsq):
        assert torch.equal(t, t.round()), f'{e.case}: the reference is not integer'
    return dict(ymax=ymax, dxmax=dxmax, sumsq=e.sumsq.max().item() / SUM_MAX, distinct=e.y.unique().numel())


def lossless(t, dtype):
    """float64 reference -> the compared type; the preconditions promise that nothing is lost"""
    r = t.to(dtype)
    assert torch.equal(r.double(), t), f'the reference does not fit {dtype} exactly (test-design error)'
    return r


def nhwc(t_nchw):
    """always a fresh tensor: the cached reference is shared between tests, and callers corrupt what this returns"""
    return t_nchw.permute(0, 2, 3, 1).clone(memory_format=torch.contiguous_format)


def silu64(v):
    return v.double() * torch.sigmoid(v.double())


def assert_exact(got, ref, what, axes=AXES_NHWC):
    """Every element of `got` equals `ref` (a float64 tensor of the same shape, laid out along `axes`; it is cast to got's type without
    loss).  Equality is of values: a NaN in `got` differs from everything, and the two zeros are the same number.  On a mismatch the message
    gives the count of wrong elements, their bounding box along each axis and the first eight (index, got, want) — enough to name the tile,
    the tap or the slab."""
    assert tuple(got.shape) == tuple(ref.shape), f'{what}: shape {tuple(got.shape)} against the reference {tuple(ref.shape)}'
    assert len(axes) == got.dim(), f'{what}: {got.dim()} dimensions, axes {axes}'
    got = got.detach().cpu()
    want = lossless(ref.detach().cpu().double(), got.dtype)
    bad = ~(got == want)
    n = int(bad.sum())
    if n == 0:
        return
    idx = bad.nonzero()
    lo, hi = idx.min(0).values.tolist(), idx.max(0).values.tolist()
    box = ', '.join(f'{a} {l}..{h}' for a, l, h in zip(axes, lo, hi))
    first = '; '.join(f'({", ".join(map(str, i.tolist()))}): got {got[tuple(i.tolist())].item()!r} want {want[tuple(i.tolist())].item()!r}' for i in idx[:8])
    raise AssertionError(f'{what}: {n} of {bad.numel()} elements differ; bounding box [{box}]; first (' + ', '.join(axes) + f') got / want: {first}')


def assert_stats_exact(slabs, e, what):
    """slabs: fp32 [n][2][K] as the kernel wrote them (any partition of the pixels).  Every slab must have been written (they start as NaN),
    and their float64 sum must equal the integer SUM y and SUM y^2 of the reference exactly."""
    slabs = slabs.detach().cpu()
    unwritten = (~torch.isfinite(slabs)).flatten(1).any(1).nonzero().flatten().tolist()
    assert not unwritten, f'{what}: {len(unwritten)} of {slabs.shape[0]} statistic slabs hold a non-finite value, the first ones {unwritten[:8]}'
    total = slabs.double().sum(0, keepdim=True)
    assert_exact(total, torch.stack([e.sum, e.sumsq]).unsqueeze(0), f'{what} (slab 0 = the sum of all {slabs.shape[0]} slabs)', AXES_STAT)


def ulps_bf16(a, b):
    """distance of a from b in units of b's bf16 ulp (8 significant bits), with b's magnitude floored at 2^-10"""
    a, b = a.double(), b.double()
    return (a - b).abs() / (b.abs().clamp_min(2.0 ** -10) * 2.0 ** -7)


def _params(fn, name):
    for m in fn.pytestmark:
        if m.name == 'parametrize' and m.args[0] == name:
            return list(m.args[1])
    raise LookupError(f'{fn.__name__} has no parameter {name}')


def case_lists():
    """The shapes the exact tests run, read from the parity tests' own lists (tests/test_gpu_kernels.py), so that a shape added there gets
    an exact test too: (conv cases, deep cases, deep weight-gradient cases, residual cases, stem shapes (N, H, W, K) of test_stem_conv,
    stem shapes of test_stem_patch_kernel_bf16)."""
    import inspect
    import test_gpu_kernels as tk
    stem = _params(tk.test_stem_conv, 'shape')
    # that test's N, H, W are set in its body, not in a list: fail here, not drift silently, if they change
    assert 'N, H, W = 3, 64, 192' in inspect.getsource(tk.test_stem_patch_kernel_bf16), 'test_stem_patch_kernel_bf16 changed its image size'
    patch = [(3, 64, 192, K) for K in _params(tk.test_stem_patch_kernel_bf16, 'K')]
    return tk.CONV_CASES, tk.DEEP_CASES, tk.WGRAD_DEEP_CASES, tk.RES_CASES, stem, patch


def round_up(n, m):
    return (n + m - 1) // m * m


def in_slice(ref_nhwc, pitch, off, poison):
    """float64 [N][H][W][pitch]: `ref_nhwc` in lanes off .. off + K of a buffer whose other lanes hold `poison` — what a whole pitched buffer
    must equal after a call that writes the channel slice only, so that one `assert_exact` covers the values and the guard lanes"""
    full = torch.full(tuple(ref_nhwc.shape[:3]) + (pitch,), float(poison), dtype=torch.float64)
    full[..., off:off + ref_nhwc.shape[3]] = ref_nhwc
    return full


def uncovered(case):
    """(first row, first column) of x that lies under no window of the case (H, W where every row / column is covered)"""
    N, H, W, C, K, R, S, stride, pad = window(case)
    return (min(H, (out_dim(H, R, stride, pad) - 1) * stride + R - pad), min(W, (out_dim(W, S, stride, pad) - 1) * stride + S - pad))


# ---- the call forms outside the backbone's and neck's layer table (tests/test_gpu_exact_forms.py), all (N, H, W, C, K, R, S, stride, pad)
# ragged K, written as a channel slice: detection logits (K = na * no), mask logits, segmentation logits; their backward pads K with zeros
RAGGED_CASES = [
    (2, 28, 28, 256, 3, 1, 1, 1, 0),
    (2, 12, 12, 64, 1, 1, 1, 1, 0),
    (2, 20, 20, 128, 27, 1, 1, 1, 0),
    (1, 8, 8, 64, 255, 1, 1, 1, 0),
    (1, 9, 11, 32, 18, 3, 3, 1, 1),
]
# 2x2 / stride 2 / pad 0: the mask head's ConvTranspose2d (its data gradient), that layer's backward (its forward) and its weight gradient
DECONV_CASES = [
    (2, 28, 28, 256, 256, 2, 2, 2, 0),       # the head's own
    (1, 10, 6, 16, 24, 2, 2, 2, 0),
    (2, 12, 20, 64, 32, 2, 2, 2, 0),
    (1, 11, 7, 16, 24, 2, 2, 2, 0),          # odd sides: the last row and the last column of x lie under no window
]
WINDOW_CASES = [
    (1, 12, 12, 16, 16, 5, 5, 1, 2),
    (2, 16, 16, 16, 32, 5, 5, 2, 2),         # parity classes of 3 and 2 taps per axis
    (2, 10, 12, 32, 32, 3, 3, 1, 0),
    (2, 12, 12, 32, 32, 3, 3, 2, 0),         # an uncovered last row and column, even sides
    (1, 13, 11, 32, 32, 3, 3, 2, 0),         # odd sides, stride 2, no padding
    (1, 8, 8, 16, 16, 3, 3, 1, 2),           # pad > R // 2: the output is larger than the input, pad' = 0 in the data gradient
    # an output row wider than the input row + 1: from a tile that begins in the last column (m = 384 = image 3, row 4, column 10 of 11) the
    # window origin of the next output row lies BEFORE the tile's — a negative offset in the generic loader, whose k-blocks are whole taps
    # here (C = 64); forward for the first, data gradient (dy is the narrow tensor, K = 64 its channels) for the second
    (4, 8, 9, 64, 16, 3, 3, 1, 2),
    (4, 10, 11, 16, 64, 3, 3, 1, 0),
    (2, 9, 12, 32, 24, 1, 3, 1, 0),          # R != S
    (2, 12, 9, 24, 32, 3, 1, 1, 1),
    (1, 11, 13, 24, 40, 5, 3, 1, 1),
    (2, 12, 12, 32, 32, 4, 4, 2, 1),         # two taps in every parity class
    (2, 14, 14, 256, 256, 3, 3, 1, 1),       # the mask head's maps: H and W are no multiples of 8
    (3, 14, 14, 64, 64, 3, 3, 1, 1),
    (1, 6, 6, 8, 8, 3, 3, 1, 1),             # the smallest legal layer: one partly filled tile in every direction
]
WINDOW_FWD_WGRAD_CASES = [(2, 12, 12, 32, 32, 1, 1, 2, 0)]      # 1x1 / stride 2: its data gradient is refused (a parity class without taps)
WINDOW_F32_CASES = [(2, 16, 16, 4, 8, 5, 5, 2, 2)]              # C = 4, fp32's vector: a 32-element k-block spans eight taps
# shapes a filter- or patch-resident family takes with a bf16 output and hands on with an fp32 one
DECLINED_CASES = [
    (2, 16, 32, 64, 64, 3, 3, 1, 1),
    (2, 32, 64, 32, 64, 3, 3, 2, 1),
    (2, 40, 40, 128, 128, 3, 3, 1, 1),
]
# refused by hdy_conv_fwd (7 x 7 = 49 taps against the loader's 31 tap bits): kept here so that its preconditions are checked all the same
REFUSED_WINDOW_CASE = (1, 20, 20, 8, 16, 7, 7, 2, 3)
# a layer the deep-pipelined family takes (with its tile minimum lifted) and the same layer with output rows wider than the input's + 1, which it must not
DEEP_CONTROL_CASE, DESCENDING_DEEP_CASE = (4, 8, 9, 64, 128, 3, 3, 1, 1), (4, 8, 9, 64, 128, 3, 3, 1, 2)
FORM_CASES = (RAGGED_CASES + DECONV_CASES + WINDOW_CASES + WINDOW_FWD_WGRAD_CASES + WINDOW_F32_CASES + DECLINED_CASES + [REFUSED_WINDOW_CASE] +
              [DEEP_CONTROL_CASE, DESCENDING_DEEP_CASE])


def all_shapes():
    """every distinct (case, stem) the exact tests build a reference for"""
    conv, deep, wdeep, res, stem, patch = case_lists()
    shapes = [(c, False) for c in list(conv) + list(deep) + list(wdeep)]
    shapes += [((N, H, W, C, K, R, 1, R // 2), False) for N, H, W, C, K, R, _, _ in res]
    shapes += [(stem_case(*s), True) for s in list(stem) + list(patch)]
    return sorted(set(shapes)) + [(c, False) for c in FORM_CASES]
