"""Bit-exact tests of every convolution kernel family on a real MI355X (the recipe, its preconditions and the comparer: tests/exact_ref.py).

The parity tests (tests/test_gpu_kernels.py) use real operands and one loose criterion — 1.5e-2 of the tensor's maximum in bf16, 1e-3 of the
largest BatchNorm sum — which one wrong product term, a border pixel read from the wrong place or a pixel counted twice in a statistics slab
passes.  Here the operands are small integers, so every product and every partial sum is exact in fp32 and in bf16, the result is independent
of summation order, split count, tile order and kernel family, and each leg is compared for equality with a float64 CPU convolution; a failure
names the coordinates (`assert_exact`).  The shapes, the option contexts and the dispatch-log assertions are the parity tests' own: an exact
test that silently ran the generic kernel would prove nothing about the specialised one.

Legs of a case: forward raw with statistic slabs (SUM y and SUM y^2 equal the integers exactly); scale / shift with accumulate; scale / shift
with a pitched residual; SiLU alone and with the residual (the pre-activation is exact, only the activation's rounding remains); ReLU; data
gradient written and accumulated; weight gradient into stacked grad_a / grad_b, written and accumulated.  Buffers as in the parity tests:
pitched channel slices with poison outside, NaN-filled packs, statistic slabs, weight-gradient workspaces and outputs that are only written.
The call forms outside the backbone's and neck's layer table (ragged K, fp32 output from bf16 operands, padded K, general windows) live in
tests/test_gpu_exact_forms.py.

Two legs are not equalities, by the kernels' design:
  * SiLU: u / (1 + exp(-u)) with the fp32 hardware exponential, then one bf16 rounding — within one bf16 ulp of the float64 value (a half-ulp
    rounding which the fp32 error can flip); fp32: within 1e-4 |ref|, plus 2^-119 absolute: below u = -88.72 exp(-u) overflows fp32 and the
    kernel returns -0 where the true value is at most 88.72 e^-88.72 = 2.6e-37.
  * SiLU with a residual, bf16: every bf16 vector epilogue stages the activated tile in LDS as bf16 and adds the residual to that (two
    roundings, as a bf16 framework's `silu(bn(conv)) + x` does), so the bound is half an ulp of SiLU(u) plus half an ulp of the sum.
"""
import os
from contextlib import ExitStack

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from hd_yolo_amd import _lib, ops  # noqa: E402
import exact_ref as X  # noqa: E402
from exact_ref import AXES_W, assert_exact, assert_stats_exact, nhwc  # noqa: E402
from test_gpu_kernels import DEV, DTYPES, expected_dispatch, to_dev_nhwc  # noqa: E402

CONV_CASES, DEEP_CASES, WGRAD_DEEP_CASES, RES_CASES, STEM_SHAPES, STEM_PATCH_SHAPES = X.case_lists()
BF16, F32 = torch.bfloat16, torch.float32
NAN = float('nan')
ALL_LEGS = ('fwd', 'acc', 'res', 'silu', 'relu', 'dgrad', 'wgrad')
DECLINE_RELU = ('conv3x3_c', 'conv3x3s2_', 'conv_stem')        # families whose kernels have no ReLU instance: they hand the call on


def dname(dtype):
    return 'bf16' if dtype == BF16 else 'fp32'


class Layer:
    """the device side of one case: operands, packs and the launches of the legs"""

    def __init__(self, e, dtype):
        self.e, self.dtype = e, dtype
        N, H, W, C, K, R, S, stride, pad = X.window(e.case)
        self.geo = (K, R, S, stride, pad)
        self.stem_hw = (H, W) if e.stem else None
        self.scale, self.shift = e.scale.float().to(DEV), e.shift.float().to(DEV)
        self.wdev = e.w.float().to(DEV)
        kind = ops.PACK_STEM if e.stem else ops.PACK_FWD
        self.wp = ops.pack_alloc(K, C, R, S, stride, pad, kind, dtype, DEV).fill_(NAN)              # the pack must write every element (padding too)
        if e.stem:
            self.xd = torch.full((N, H + 4, W + 4, 4), NAN, dtype=dtype, device=DEV)                # the prep pass must write every element
            ops.run([ops.rec_stem_prep(e.x.float().to(DEV), self.xd), ops.rec_pack(self.wdev, None, stride, pad, kind, self.wp)])
        else:
            self.xd = to_dev_nhwc(e.x, dtype, ld=C + 16, off=8)
            ops.run([ops.rec_pack(self.wdev, None, stride, pad, kind, self.wp)])

    def forward(self, affine=False, act=ops.ACT_NONE, prefill=None, res=None, stats=None):
        """one forward launch into a pitched slice: NaN where the call only writes, `prefill` where it accumulates; (y on the CPU, dispatch log)"""
        e, dtype = self.e, self.dtype
        N, K = e.case[0], e.case[4]
        ybuf = torch.full((N, e.Ho, e.Wo, K + 8), 5.0, dtype=dtype, device=DEV)
        y = ybuf[..., 8:]
        if prefill is None:
            y.fill_(NAN)
        else:
            y.copy_(nhwc(prefill).to(dtype))
        resd = None if res is None else to_dev_nhwc(res, dtype, ld=K + 24, off=16)
        _lib.dispatch_log(reset=True)
        ops.run([ops.rec_conv_fwd(self.xd, self.wp, y, *self.geo, scale=self.scale if affine else None, shift=self.shift if affine else None, stats=stats,
                                  act=act, accumulate=prefill is not None, res=resd, stem_hw=self.stem_hw)])
        log = _lib.dispatch_log(reset=True)
        assert (ybuf[..., :8].float() == 5.0).all(), 'wrote outside the channel slice'
        if resd is not None:
            assert torch.equal(resd.cpu().double(), nhwc(res)), 'the residual operand was modified'
        return y.cpu(), log


def check_silu(got, u, res, dtype, what):
    """got against SiLU(u) (+ res) evaluated in float64, u exact; the bounds are derived in the module docstring"""
    s = X.silu64(nhwc(u))
    ref = s if res is None else s + nhwc(res)
    err = (got.double() - ref).abs()
    assert torch.isfinite(got).all(), f'{what}: non-finite output'
    if dtype == BF16:
        ulp = lambda b: b.abs().clamp_min(2.0 ** -10) * 2.0 ** -7
        bound = 1.01 * ulp(ref) if res is None else 1.01 * 0.5 * (ulp(s) + ulp(ref))
    else:
        bound = 1e-4 * ref.abs() + 2.0 ** -119
    ratio = err / bound
    i = ratio.argmax()
    idx = tuple(int(v) for v in torch.unravel_index(i, ratio.shape))
    print(f'{what}: worst error / bound = {ratio.flatten()[i].item():.3f} at (n, y, x, channel) = {idx}')
    assert ratio.flatten()[i].item() <= 1.0, (f'{what}: {int((ratio > 1).sum())} elements beyond the bound, the worst {ratio.flatten()[i].item():.2f} x at (n, y, x, channel) '
                                              f'= {idx}: got {got[idx].item()!r}, want {ref[idx].item()!r}')


def exact_conv(case, dtype, legs=ALL_LEGS, stem=False, fwd_family=None, relu_family=None, prepare=None):
    """The legs of one case against the float64 reference.  `fwd_family`: what the dispatch log of every forward leg but ReLU must contain
    (a string, or a predicate of the log); `relu_family`: the same for the ReLU leg (default: none of the families without a ReLU instance).
    `prepare`: called with the Layer before its first launch (tests/test_gpu_exact_forms.py poisons what no window covers).
    Returns the logs of (forward with statistics, data gradient, weight gradient) like the parity tests' conv_case."""
    e = X.reference(case, stem)
    X.check_preconditions(e)
    N, H, W, C, K, R, S, stride, pad = X.window(case)
    Ho, Wo = e.Ho, e.Wo
    tag = f'{case} {dname(dtype)}'
    L = Layer(e, dtype)
    if prepare is not None:
        prepare(L)

    def ran(log, want, what):
        if want is None:
            return
        ok = want(log) if callable(want) else any(want in n for n in log)
        assert ok, f'{tag} {what} ran {log}' + ('' if callable(want) else f', expected {want}')

    log_fwd, log_dgrad, log_wgrad = [], [], []
    if 'fwd' in legs:
        mt = ops.stat_slabs(N, H, W, C, K, R, S, stride, pad, dtype)
        stats = torch.full((mt + 1, 2, K), NAN, dtype=torch.float32, device=DEV)                # every slab must be written, and none behind them
        y, log_fwd = L.forward(stats=stats[:mt])
        ran(log_fwd, fwd_family, 'forward with statistics')
        assert_exact(y, nhwc(e.y), f'{tag} forward {log_fwd}')
        assert_stats_exact(stats[:mt], e, f'{tag} statistics {log_fwd}')
        assert torch.isnan(stats[mt]).all(), 'wrote behind the last statistics slab'
    if 'acc' in legs:
        y, log = L.forward(affine=True, prefill=e.acc)
        ran(log, None if stem else fwd_family, 'scale / shift / accumulate')                    # the patch-resident stem kernel does not accumulate
        assert_exact(y, nhwc(e.affine + e.acc), f'{tag} scale / shift / accumulate {log}')
        if stem:
            y, log = L.forward(affine=True)
            ran(log, fwd_family, 'scale / shift')
            assert_exact(y, nhwc(e.affine), f'{tag} scale / shift {log}')
    if 'res' in legs and not stem:
        y, log = L.forward(affine=True, res=e.res)
        ran(log, fwd_family, 'scale / shift / residual')
        assert_exact(y, nhwc(e.affine + e.res), f'{tag} scale / shift / residual {log}')
    if 'silu' in legs:
        y, log = L.forward(affine=True, act=ops.ACT_SILU)
        ran(log, fwd_family, 'SiLU')
        check_silu(y, e.affine, None, dtype, f'{tag} SiLU {log}')
        if not stem:
            y, log = L.forward(affine=True, act=ops.ACT_SILU, res=e.res)
            ran(log, fwd_family, 'SiLU with residual')
            check_silu(y, e.affine, e.res, dtype, f'{tag} SiLU with residual {log}')
    if 'relu' in legs:
        y, log = L.forward(affine=True, act=ops.ACT_RELU)
        ran(log, relu_family or (lambda g: len(g) == 1 and not any(g[0].startswith(d) for d in DECLINE_RELU)), 'ReLU')
        assert_exact(y, nhwc(F.relu(e.affine)), f'{tag} ReLU {log}')
    if stem:
        if 'wgrad' in legs:
            log_wgrad = wgrad_legs(e, L.xd, to_dev_nhwc(e.dy, dtype), dtype, tag, stem_hw=(H, W))
        return log_fwd, log_dgrad, log_wgrad
    ve = 8 if dtype == BF16 else 4                                  # the gradient kernels move whole vectors of channels
    if K % ve or C % ve or not ('dgrad' in legs or 'wgrad' in legs):
        return log_fwd, log_dgrad, log_wgrad
    dyd = to_dev_nhwc(e.dy, dtype, ld=K + 8, off=0)
    if 'dgrad' in legs:
        wpd = ops.pack_alloc(K, C, R, S, stride, pad, ops.PACK_DGRAD, dtype, DEV).fill_(NAN)
        ops.run([ops.rec_pack(L.wdev, None, stride, pad, ops.PACK_DGRAD, wpd)])
        dxbuf = torch.full((N, H, W, C + 8), 5.0, dtype=dtype, device=DEV)
        dx = dxbuf[..., 8:]
        dx.fill_(NAN)
        _lib.dispatch_log(reset=True)
        ops.run([ops.rec_conv_dgrad(dyd, wpd, dx, R, S, stride, pad)])
        log_dgrad = _lib.dispatch_log(reset=True)
        assert_exact(dx.cpu(), nhwc(e.dx), f'{tag} data gradient {log_dgrad}')
        assert (dxbuf[..., :8].float() == 5.0).all(), 'the data gradient wrote outside the channel slice'
        dx2 = nhwc(e.dx_acc).to(dtype).to(DEV)
        ops.run([ops.rec_conv_dgrad(dyd, wpd, dx2, R, S, stride, pad, accumulate=True)])
        log2 = _lib.dispatch_log(reset=True)
        assert log2 == log_dgrad, f'{tag}: the accumulating data gradient ran {log2}, the writing one {log_dgrad}'
        assert_exact(dx2.cpu(), nhwc(e.dx + e.dx_acc), f'{tag} data gradient, accumulated {log2}')
    if 'wgrad' in legs:
        log_wgrad = wgrad_legs(e, L.xd, dyd, dtype, tag)
    return log_fwd, log_dgrad, log_wgrad


def wgrad_legs(e, xd, dyd, dtype, tag, stem_hw=None):
    N, H, W, C, K, R, S, stride, pad = X.window(e.case)
    ws = torch.full((ops.wgrad_ws_bytes(N, H, W, C, K, R, S, stride, pad, dtype, stem=stem_hw is not None) // 4 + 1,), NAN, dtype=torch.float32, device=DEV)
    ka = K // 2 if K >= 16 else K
    ga = torch.full((ka, C, R, S), NAN, dtype=torch.float32, device=DEV)
    gb = torch.full((K - ka, C, R, S), NAN, dtype=torch.float32, device=DEV) if ka < K else None
    logs = []
    for acc in (False, True):
        if acc:
            ws.fill_(NAN)                           # read only where written, in this call
            ga.zero_()
            if gb is not None:
                gb.fill_(2.0)
        _lib.dispatch_log(reset=True)
        ops.run([ops.rec_conv_wgrad(xd, dyd, ga, gb, R, S, stride, pad, ws, accumulate=acc, stem_hw=stem_hw)])
        logs.append(_lib.dispatch_log(reset=True))
        how = 'accumulated' if acc else 'written'
        assert_exact(ga.cpu(), e.dw[:ka], f'{tag} weight gradient a, {how} {logs[-1]}', AXES_W)
        if gb is not None:
            assert_exact(gb.cpu(), e.dw[ka:] + (2.0 if acc else 0.0), f'{tag} weight gradient b, {how} {logs[-1]}', AXES_W)
    assert logs[0] == logs[1], f'{tag}: the accumulating weight gradient ran {logs[1]}, the writing one {logs[0]}'
    return logs[0]


# case-major order: both types of a case share one CPU reference (exact_ref.reference keeps the last two)
@pytest.mark.parametrize('case,dtype', [(c, d) for c in CONV_CASES for d in DTYPES],
                         ids=[f'case{i}-{dname(d)}' for i in range(len(CONV_CASES)) for d in DTYPES])
def test_conv_exact(case, dtype):
    want = expected_dispatch(case) if dtype == BF16 else (None, None, None)
    logs = exact_conv(case, dtype, fwd_family=want[0])
    for got, w, what in zip(logs, want, ('forward', 'data gradient', 'weight gradient')):
        if w is not None:
            assert w in got, f'{what} of {case} ran {got}, expected {w}'


def deep_options(bn, **more):
    opts = dict(HDY_DEEP_MIN_TILES=1, HDY_DEEP_BN=bn, HDY_DEEP_ALL=1, HDY_DEEP_WALK=1)
    opts.update(more)
    return opts


def with_options(opts):
    es = ExitStack()
    for k, v in opts.items():
        if v is not None:
            es.enter_context(_lib.option(k, v))
    return es


@pytest.mark.parametrize('case,bn', [(c, bn) for c in DEEP_CASES for bn in (0, 128, 256)],
                         ids=[f'case{i}-bn{bn}' for i in range(len(DEEP_CASES)) for bn in (0, 128, 256)])
def test_deep_pipelined_conv_exact(case, bn):
    """conv_deep.hip on the shapes and under the switches of test_deep_pipelined_conv: both column tiles, forward with BatchNorm sums, every
    epilogue, the stride-1 data gradient and the stride-2 class walk (HDY_DEEP_WALK = 1, default, 0), and the same forward through the generic
    kernel (HDY_NO_DEEP)."""
    N, H, W, C, K, R, stride, pad = case
    deep = lambda log: len(log) == 1 and log[0].startswith('deep_256x')
    with with_options(deep_options(bn)):
        log_fwd, log_dgrad, _ = exact_conv(case, BF16, fwd_family=deep, relu_family=deep)
    assert log_fwd == ['deep_256x128'], log_fwd                  # statistics: 128-wide instances
    if stride == 1 and K % 64 == 0 and C >= 128:
        assert log_dgrad and log_dgrad[0].startswith('deep_256x'), log_dgrad
    if stride == 2 and K % 64 == 0 and C >= 128:
        assert log_dgrad and log_dgrad[0].startswith('deep_256x') and log_dgrad[0].endswith('_walk'), log_dgrad
        with with_options(dict(HDY_DEEP_MIN_TILES=1)):           # default (HDY_DEEP_WALK = 2): the deep pipeline from 256 gradient channels out, else the generic kernel's walk
            assert exact_conv(case, BF16, legs=('dgrad',))[1][0].startswith('deep_256x' if C >= 256 else 'igemm_')
        with with_options(dict(HDY_DEEP_MIN_TILES=1, HDY_DEEP_WALK=0)):
            assert exact_conv(case, BF16, legs=('dgrad',))[1][0].startswith('igemm_')
    with with_options(deep_options(bn, HDY_NO_DEEP=1)):
        log_fwd, _, _ = exact_conv(case, BF16, legs=('fwd',))
    assert log_fwd and not any(n.startswith('deep_') for n in log_fwd), log_fwd


@pytest.mark.parametrize('case,off', [(c, off) for c in WGRAD_DEEP_CASES for off in (0, 1)],
                         ids=[f'case{i}-{"generic" if off else "deep"}' for i in range(len(WGRAD_DEEP_CASES)) for off in (0, 1)])
def test_deep_pipelined_weight_gradient_exact(case, off):
    """conv_wgrad_deep.hip and, on the same operands, the kernel that takes the shape without it (HDY_NO_WGRAD_DEEP): stacked gradients,
    written and accumulated, pitched x and dy; with the deep kernel also every other leg of the layer"""
    with _lib.option('HDY_NO_WGRAD_DEEP', off):
        _, _, log_w = exact_conv(case, BF16, legs=('wgrad',) if off else ALL_LEGS)
    assert ('wgrad_deep' in log_w) == (off == 0), log_w


@pytest.mark.parametrize('case', RES_CASES, ids=[f'{c[6]}-{c[3]}x{c[4]}k{c[5]}' for c in RES_CASES])
def test_conv_eval_epilogue_with_residual_exact(case):
    """the residual operand (a pitched slice) in every kernel family's epilogue, under the options of test_conv_eval_epilogue_with_residual"""
    N, H, W, C, K, R, want, opts = case
    with with_options(opts):
        exact_conv((N, H, W, C, K, R, 1, R // 2), BF16, legs=('acc', 'res', 'silu'), fwd_family=want)


def stem_families(N, H, W, K, dtype):
    """the patch-resident stem kernels take bf16, K = 16 .. 64 in steps of 16 and outputs that are multiples of 16 x 32"""
    fits = dtype == BF16 and K % 16 == 0 and 16 <= K <= 64 and (H // 2) % 16 == 0 and (W // 2) % 32 == 0
    fwd = fits and not os.environ.get('HDY_NO_STEM_KERNEL')
    return (lambda log: ('conv_stem' in log) == bool(fwd)), fits


@pytest.mark.parametrize('shape,dtype', [(s, d) for s in STEM_SHAPES for d in DTYPES],
                         ids=['x'.join(map(str, s)) + '-' + dname(d) for s in STEM_SHAPES for d in DTYPES])
def test_stem_conv_exact(shape, dtype):
    """the 6x6 / stride-2 stem on the shapes of test_stem_conv: forward with statistics and every epilogue the stem accepts, weight gradient
    (generic kernel + split reduction in fp32 and for the ineligible size, the patch-resident kernel in bf16)"""
    N, H, W, K = shape
    fwd, fits = stem_families(N, H, W, K, dtype)
    _, _, log_w = exact_conv(X.stem_case(*shape), dtype, stem=True, fwd_family=fwd, relu_family=lambda log: 'conv_stem' not in log)
    if not os.environ.get('HDY_NO_STEM_WGRAD'):
        assert ('wgrad_stem' in log_w) == fits, log_w


@pytest.mark.parametrize('shape', STEM_PATCH_SHAPES, ids=[f'K{s[3]}' for s in STEM_PATCH_SHAPES])
def test_stem_patch_kernel_exact(shape):
    """the shapes of test_stem_patch_kernel_bf16: 18 tiles of 16 x 32 outputs, one statistics slab per workgroup"""
    N, H, W, K = shape
    fwd, _ = stem_families(N, H, W, K, BF16)
    if not os.environ.get('HDY_NO_STEM_KERNEL'):
        assert ops.stat_slabs(N, H, W, 3, K, 6, 6, 2, 2, BF16) == N * (H // 32) * (W // 64)
    exact_conv(X.stem_case(*shape), BF16, stem=True, legs=('fwd', 'acc', 'silu', 'relu'), fwd_family=fwd, relu_family=lambda log: 'conv_stem' not in log)
