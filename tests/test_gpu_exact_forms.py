"""Bit-exact tests of the convolution entry points in the forms the backbone's and neck's layer table (CONV_CASES) does not hold: the heads'
own calls and the rest of the window space the C ABI accepts (the recipe, its preconditions and the comparer: tests/exact_ref.py; the device
side of a layer and the legs of a whole case: tests/test_gpu_exact.py).

  a  ragged K written as a channel slice (detection, mask and segmentation logits): the scalar epilogue with raw, bias-only, bias + ReLU,
     scale / shift, accumulate and residual; and fp32 output from bf16 operands (`out_f32`)
  b  the backward of those layers: K padded with zero channels to a multiple of 8 in the pack, in dy and in the weight gradient
  c  2x2 / stride 2 / pad 0 (the mask head's ConvTranspose2d) as forward, data gradient and weight gradient
  d  general windows: 5x5, 4x4 / stride 2, R != S, no padding, pad > R // 2, 1x1 / stride 2, 14 x 14 maps, the smallest layer, C = 4 in fp32,
     the backward of 7x7 / stride 2, and outputs wider than their input over several tiles (window origins that run backwards in memory)
  e  a call a filter- or patch-resident family declines (fp32 output) arrives at another kernel and is exact there
  f  what is not served raises, launches nothing and leaves the output as it was

Every comparison is an equality with the float64 CPU reference (`assert_exact`).  A buffer that a call only writes starts as NaN; a pitched
buffer is compared as a whole, so the same equality covers the slice and the poison in the lanes around it (`exact_ref.in_slice`).  What no
window of a layer covers (the last row and column of x under 2x2 / stride 2 with odd sides, for one) holds NaN in x: reading it shows in
the forward result and in the weight gradient."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from hd_yolo_amd import _lib, ops  # noqa: E402
import exact_ref as X  # noqa: E402
from exact_ref import AXES_W, assert_exact, nhwc, round_up  # noqa: E402
from test_gpu_exact import BF16, F32, NAN, Layer, deep_options, dname, exact_conv, with_options  # noqa: E402
from test_gpu_kernels import DEV, DTYPES  # noqa: E402

POISON, RES_POISON = 5.0, 7.0
# every name the convolution launchers write into the dispatch log
KNOWN = ('igemm_', 'deep_256x', 'conv3x3_c', 'conv3x3s2_c', 'dgrad3x3s2_k', 'conv_stem', 'wgrad_generic', 'wgrad3x3', 'wgrad_deep', 'wgrad_stem',
         'wgrad_reduce')
RESIDENT = ('conv3x3_c', 'conv3x3s2_c', 'dgrad3x3s2_k', 'conv_stem')       # the filter- and patch-resident families


def known(log, what):
    assert log, f'{what}: nothing was launched'
    assert all(n.startswith(KNOWN) for n in log), f'{what} ran {log}'
    return True


def only_igemm(log):
    return bool(log) and all(n.startswith('igemm_') for n in log)


def ids(cases, dtypes):
    return [f'{"x".join(map(str, c))}-{dname(d)}' for c in cases for d in dtypes]


def params(cases, dtypes=DTYPES):
    # case-major order: both types of a case share one CPU reference (exact_ref.reference keeps the last two)
    return dict(argnames='case,dtype', argvalues=[(c, d) for c in cases for d in dtypes], ids=ids(cases, dtypes))


def poison_uncovered(L):
    """NaN in the rows and columns of x behind the last window"""
    h1, w1 = X.uncovered(L.e.case)
    L.xd[:, h1:] = NAN
    L.xd[:, :, w1:] = NAN


def forward_slice(L, want, what, ydtype=None, pitch=None, off=0, scale=None, shift=None, act=ops.ACT_NONE, prefill=None, res=None, res_pitch=None,
                  res_off=0):
    """One forward launch of layer L into lanes off .. off + K of a buffer of `pitch` lanes (NaN where the call only writes, `prefill` where it
    accumulates, POISON around the slice); `want` is the NCHW float64 result.  Returns the dispatch log."""
    e = L.e
    N, K = e.case[0], e.case[4]
    ydtype = ydtype or L.dtype
    pitch = pitch or round_up(K, 8)
    ybuf = torch.full((N, e.Ho, e.Wo, pitch), POISON, dtype=ydtype, device=DEV)
    y = ybuf[..., off:off + K]
    if prefill is None:
        y.fill_(NAN)
    else:
        y.copy_(nhwc(prefill).to(ydtype))
    rbuf = resd = None
    if res is not None:
        rbuf = torch.full((N, e.Ho, e.Wo, res_pitch), RES_POISON, dtype=ydtype, device=DEV)
        resd = rbuf[..., res_off:res_off + K]
        resd.copy_(nhwc(res).to(ydtype))
    _lib.dispatch_log(reset=True)
    ops.run([ops.rec_conv_fwd(L.xd, L.wp, y, *L.geo, scale=scale, shift=shift, act=act, accumulate=prefill is not None, res=resd)])
    log = _lib.dispatch_log(reset=True)
    what = f'{e.case} {dname(L.dtype)} -> {dname(ydtype)}, lanes {off}..{off + K} of {pitch}: {what} {log}'
    print(what)
    known(log, what)
    assert_exact(ybuf.cpu(), X.in_slice(nhwc(want), pitch, off, POISON), what)
    if rbuf is not None:
        assert_exact(rbuf.cpu(), X.in_slice(nhwc(res), res_pitch, res_off, RES_POISON), what + ': the residual operand')
    return log


def col(v):
    return v.view(1, -1, 1, 1)


# ------------------------------------------------------------------------------------------------------------------------ a: ragged K
@pytest.mark.parametrize(**params(X.RAGGED_CASES))
def test_ragged_k_into_a_channel_slice(case, dtype):
    """K = 3, 1, 27, 255, 18 into buf[..., :K] of a pitch of round_up(K, 8) lanes — and, in fp32, into lanes 1 .. 1 + K of K + 3 (rows that
    are not 16-byte aligned).  The residual has a ragged pitch of its own (K + 5, from lane 2)."""
    e = X.reference(case)
    X.check_preconditions(e)
    K = case[4]
    L = Layer(e, dtype)
    sc, sh = L.scale, L.shift
    for pitch, off in [(round_up(K, 8), 0)] + ([(K + 3, 1)] if dtype == F32 else []):
        go = lambda want, what, **kw: forward_slice(L, want, what, pitch=pitch, off=off, **kw)
        go(e.y, 'raw')
        go(e.y + col(e.shift), 'shift only', shift=sh)
        go(F.relu(e.y + col(e.shift)), 'shift + ReLU', shift=sh, act=ops.ACT_RELU)
        go(e.affine, 'scale + shift', scale=sc, shift=sh)
        go(e.affine + e.acc, 'scale + shift, accumulated', scale=sc, shift=sh, prefill=e.acc)
        go(e.affine + e.res, 'scale + shift + residual', scale=sc, shift=sh, res=e.res, res_pitch=K + 5, res_off=2)


@pytest.mark.parametrize('case', X.RAGGED_CASES, ids=ids(X.RAGGED_CASES, [BF16]))
def test_ragged_k_fp32_output_from_bf16_operands(case):
    """`out_f32`: the accumulator goes through the epilogue to an fp32 store and is never a bf16 value.  With the bias raised to about 300 the
    results are integers and half-integers beyond 256: exact in fp32 (24 significant bits), not in bf16 (8 bits: only every second integer
    from 256 on), so a kernel that rounded through bf16 before the store fails the equality."""
    e = X.reference(case)
    X.check_preconditions(e)
    L = Layer(e, BF16)
    big = e.shift + 300.0
    bigd = big.float().to(DEV)
    go = lambda want, what, **kw: forward_slice(L, want, what, ydtype=F32, **kw)
    go(e.y, 'raw')
    go(F.relu(e.y + col(e.shift)), 'shift + ReLU', shift=L.shift, act=ops.ACT_RELU)
    for want, what, kw in ((e.y + col(big), 'shift only, near 300', dict(shift=bigd)),
                           (e.y * col(e.scale) + col(big), 'scale + shift near 300', dict(scale=L.scale, shift=bigd)),
                           (F.relu(e.y * col(e.scale) + col(big)), 'scale + shift near 300 + ReLU', dict(scale=L.scale, shift=bigd, act=ops.ACT_RELU))):
        assert (want.abs() > 256).any() and (want.to(BF16).double() != want).any(), f'{case} {what}: every expected value is a bf16 value (test-design error)'
        go(want, what, **kw)


# ------------------------------------------------------------------------------------------------------------------------ b: padded K
def bits(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


@pytest.mark.parametrize(**params(X.RAGGED_CASES))
def test_zero_padded_k_in_the_backward(case, dtype):
    """The backward of a ragged-K layer runs on Kp = round_up(K, 8) channels, the last Kp - K of them zero: in the pack (K = Kp rows from a
    weight of K), in dy, and in the weight gradient (fewer gradient rows than dy has channels, or Kp rows of which the last are zero)."""
    e = X.reference(case)
    X.check_preconditions(e)
    N, H, W, C, K, R, S, stride, pad = case
    Kp = round_up(K, 8)
    tag = f'{case} {dname(dtype)}'
    L = Layer(e, dtype)
    wcat = torch.cat([L.wdev, torch.zeros((Kp - K, C, R, S), dtype=torch.float32, device=DEV)])
    packs = {}
    for kind, name in ((ops.PACK_FWD, 'forward'), (ops.PACK_DGRAD, 'data-gradient')):
        p1 = ops.pack_alloc(Kp, C, R, S, stride, pad, kind, dtype, DEV).fill_(NAN)
        p2 = ops.pack_alloc(Kp, C, R, S, stride, pad, kind, dtype, DEV).fill_(NAN)
        ops.run([ops.rec_pack(L.wdev, None, stride, pad, kind, p1, K=Kp), ops.rec_pack(wcat, None, stride, pad, kind, p2)])
        assert not torch.isnan(p2).any(), f'{tag}: the {name} pack left elements unwritten'
        assert torch.equal(bits(p1), bits(p2)), f'{tag}: the {name} pack of K = {K} rows padded to {Kp} differs from the pack of cat([w, zeros])'
        packs[kind] = p1

    # dy: Kp channels in a pitch of Kp + 8, zeros in K .. Kp
    dybuf = torch.full((N, e.Ho, e.Wo, Kp + 8), RES_POISON, dtype=dtype, device=DEV)
    dyd = dybuf[..., :Kp]
    dyd.zero_()
    dyd[..., :K] = nhwc(e.dy).to(dtype)
    dxbuf = torch.full((N, H, W, C + 8), POISON, dtype=dtype, device=DEV)
    dx = dxbuf[..., 8:]
    for acc in (False, True):
        if acc:
            dx.copy_(nhwc(e.dx_acc).to(dtype))
        else:
            dx.fill_(NAN)
        _lib.dispatch_log(reset=True)
        ops.run([ops.rec_conv_dgrad(dyd, packs[ops.PACK_DGRAD], dx, R, S, stride, pad, accumulate=acc)])
        log = _lib.dispatch_log(reset=True)
        what = f'{tag} data gradient from {Kp} channels, {"accumulated" if acc else "written"} {log}'
        print(what)
        assert known(log, what) and only_igemm(log), what
        assert_exact(dxbuf.cpu(), X.in_slice(nhwc(e.dx + (e.dx_acc if acc else 0.0)), C + 8, 8, POISON), what)

    ws = torch.full((ops.wgrad_ws_bytes(N, H, W, C, Kp, R, S, stride, pad, dtype) // 4 + 1,), NAN, dtype=torch.float32, device=DEV)
    zrows, behind = torch.zeros((Kp - K, C, R, S), dtype=torch.float64), torch.zeros((1, C, R, S), dtype=torch.float64)
    # form 1: K gradient rows from Kp channels of dy; form 2: Kp rows, the last Kp - K of them zero (written) or as found (accumulated);
    # a guard row behind both
    for rows, ref in ((K, torch.cat([e.dw, behind])), (Kp, torch.cat([e.dw, zrows, behind]))):
        gbuf = torch.full((rows + 1, C, R, S), NAN, dtype=torch.float32, device=DEV)
        ga = gbuf[:rows]
        guard = torch.zeros_like(ref)
        guard[rows:] = POISON
        for acc in (False, True):
            ws.fill_(NAN)                           # read only where written, in this call
            if acc:
                ga.fill_(2.0)
            gbuf[rows:] = POISON
            _lib.dispatch_log(reset=True)
            ops.run([ops.rec_conv_wgrad(L.xd, dyd, ga, None, R, S, stride, pad, ws, accumulate=acc)])
            log = _lib.dispatch_log(reset=True)
            what = f'{tag} weight gradient, {rows} rows from {Kp} channels, {"accumulated" if acc else "written"} {log}'
            print(what)
            known(log, what)
            prior = torch.zeros_like(ref)
            prior[:rows] = 2.0 if acc else 0.0
            assert_exact(gbuf.cpu(), ref + guard + prior, what, AXES_W)


# ------------------------------------------------------------------------------------------------------------------------ c: 2x2 / stride 2
@pytest.mark.parametrize(**params(X.DECONV_CASES))
def test_2x2_stride_2_in_all_three_roles(case, dtype):
    """Forward with statistic slabs, data gradient (written and accumulated: with odd sides the last row and column of dx are zeros, or
    what was there) and stacked weight gradient.  Even sides: the data gradient is one launch walking the four one-tap parity classes; odd
    sides: one launch per class."""
    H, W = case[1], case[2]
    log_fwd, log_dgrad, log_wgrad = exact_conv(case, dtype, legs=('fwd', 'dgrad', 'wgrad'), fwd_family=only_igemm, prepare=poison_uncovered)
    print(f'{case} {dname(dtype)}: forward {log_fwd}, data gradient {log_dgrad}, weight gradient {log_wgrad}')
    for log, what in ((log_fwd, 'forward'), (log_dgrad, 'data gradient'), (log_wgrad, 'weight gradient')):
        known(log, f'{case} {what}')
    if H % 2 == 0 and W % 2 == 0:
        assert len(log_dgrad) == 1 and log_dgrad[0].endswith('_walk'), log_dgrad
    else:
        assert len(log_dgrad) == 4 and only_igemm(log_dgrad) and not any(n.endswith('_walk') for n in log_dgrad), log_dgrad


# ------------------------------------------------------------------------------------------------------------------------ d: general windows
WINDOW_LEGS = ('fwd', 'acc', 'relu', 'dgrad', 'wgrad')
WINDOW_PARAMS = ([(c, d, WINDOW_LEGS) for c in X.WINDOW_CASES for d in DTYPES] +
                 [(c, d, ('fwd', 'acc', 'relu', 'wgrad')) for c in X.WINDOW_FWD_WGRAD_CASES for d in DTYPES] +
                 [(c, F32, WINDOW_LEGS) for c in X.WINDOW_F32_CASES] +
                 # 7x7 / stride 2: the forward pass is refused (49 taps, see the refusals below); its parity classes have 4 x 4 taps at the most
                 [(X.REFUSED_WINDOW_CASE, d, ('dgrad', 'wgrad')) for d in DTYPES])


@pytest.mark.parametrize('case,dtype,legs', WINDOW_PARAMS, ids=[f'{"x".join(map(str, c))}-{dname(d)}' for c, d, _ in WINDOW_PARAMS])
def test_general_windows(case, dtype, legs):
    """No filter- or patch-resident family and no deep-pipelined plan admits any of these shapes (windows other than 3x3 / pad 1, sides that
    are no multiples of 8, too few tiles), so the forward pass and the data gradient are the generic kernel's; the weight gradient of the
    14 x 14 maps in bf16 may be the patch-resident 3x3 kernel's, every other one is the generic kernel's."""
    log_fwd, log_dgrad, log_wgrad = exact_conv(case, dtype, legs=legs, fwd_family=only_igemm, relu_family=only_igemm, prepare=poison_uncovered)
    print(f'{case} {dname(dtype)}: forward {log_fwd}, data gradient {log_dgrad}, weight gradient {log_wgrad}')
    for log, leg, what in ((log_fwd, 'fwd', 'forward'), (log_dgrad, 'dgrad', 'data gradient'), (log_wgrad, 'wgrad', 'weight gradient')):
        if leg in legs:
            known(log, f'{case} {what}')
    assert (only_igemm(log_fwd) or 'fwd' not in legs) and (only_igemm(log_dgrad) or 'dgrad' not in legs), (log_fwd, log_dgrad)
    resident3x3 = dtype == BF16 and case[5:] == (3, 3, 1, 1) and case[3] % 32 == 0 and case[4] % 32 == 0
    assert log_wgrad[0] in (('wgrad3x3', 'wgrad_generic') if resident3x3 else ('wgrad_generic',)) and all(n.startswith('wgrad_reduce') for n in log_wgrad[1:]), log_wgrad


def test_deep_pipeline_leaves_descending_windows_to_the_generic_kernel():
    """The deep-pipelined family (opened to small layers as in test_deep_pipelined_conv_exact) reads with the same unsigned row offsets as the
    generic kernel's whole-tap loader: it takes the layer with pad 1 and must leave the same layer with pad 2 — output rows two pixels wider
    than the input's — to the generic kernel's per-lane form.  Both are exact."""
    deep = lambda log: len(log) == 1 and log[0].startswith('deep_256x')
    with with_options(deep_options(0)):
        log_fwd, _, _ = exact_conv(X.DEEP_CONTROL_CASE, BF16, legs=('fwd', 'acc', 'relu'), fwd_family=deep, relu_family=deep)
        assert deep(log_fwd), log_fwd
        log_fwd, log_dgrad, _ = exact_conv(X.DESCENDING_DEEP_CASE, BF16, legs=('fwd', 'acc', 'relu', 'dgrad'), fwd_family=only_igemm, relu_family=only_igemm)
        assert only_igemm(log_fwd) and log_dgrad and not any(n.startswith(RESIDENT) for n in log_dgrad), (log_fwd, log_dgrad)


# ------------------------------------------------------------------------------------------------------------------------ e: declined calls
@pytest.mark.parametrize('case,family', list(zip(X.DECLINED_CASES, ('conv3x3_c64', 'conv3x3s2_c32', 'conv3x3_c128'))),
                         ids=ids(X.DECLINED_CASES, [BF16]))
def test_a_declined_call_is_handed_on(case, family):
    """bf16 operands: with a bf16 output the shape is the resident family's (asserted, or the rest would prove nothing); with an fp32 output that
    family declines, and the call must arrive at a kernel that serves it — exactly."""
    e = X.reference(case)
    X.check_preconditions(e)
    L = Layer(e, BF16)
    y, log = L.forward()
    assert log == [family], f'{case} with a bf16 output ran {log}, expected {family}'
    assert_exact(y, nhwc(e.y), f'{case} bf16 output {log}')
    K = case[4]
    big = e.shift + 300.0
    for want, what, kw in ((e.y, 'raw', {}), (e.y * col(e.scale) + col(big), 'scale + shift near 300', dict(scale=L.scale, shift=big.float().to(DEV)))):
        log = forward_slice(L, want, what, ydtype=F32, pitch=K + 8, off=8, **kw)
        assert not any(n.startswith(RESIDENT) for n in log), f'{case} with an fp32 output ran {log}'


# ------------------------------------------------------------------------------------------------------------------------ f: refusals
def refused(records, message, outputs, what):
    """the launch list raises HdyError with `message`, starts nothing and leaves the NaN-filled outputs as they were"""
    _lib.dispatch_log(reset=True)
    with pytest.raises(_lib.HdyError, match=message):
        ops.run(records)
    log = _lib.dispatch_log(reset=True)
    assert log == [], f'{what}: refused, but ran {log}'
    for t in outputs:
        assert torch.isnan(t).all(), f'{what}: refused, but wrote its output'


@pytest.mark.parametrize('dtype', DTYPES, ids=dname)
def test_what_is_not_served_refuses_loudly_and_launches_nothing(dtype):
    nan = lambda *shape, dt=dtype: torch.full(shape, NAN, dtype=dt, device=DEV)
    val = lambda *shape: torch.ones(shape, dtype=dtype, device=DEV)
    w = lambda K, C, R, S: torch.ones((K, C, R, S), dtype=torch.float32, device=DEV)

    # the data gradient of 1x1 / stride 2 / pad 0: the odd rows and columns of dx belong to parity classes that no tap reaches
    wpd = ops.pack_alloc(32, 32, 1, 1, 2, 0, ops.PACK_DGRAD, dtype, DEV)
    ops.run([ops.rec_pack(w(32, 32, 1, 1), None, 2, 0, ops.PACK_DGRAD, wpd)])
    dx = nan(2, 12, 12, 32)
    refused([ops.rec_conv_dgrad(val(2, 6, 6, 32), wpd, dx, 1, 1, 2, 0)], 'leaves a parity class without taps', [dx], 'data gradient of 1x1 / stride 2')

    wp = nan(ops.pack_alloc(16, 16, 3, 3, 1, 1, ops.PACK_FWD, dtype, DEV).numel())
    refused([ops.rec_pack(w(16, 16, 3, 3), None, 3, 1, ops.PACK_FWD, wp)], 'conv_pack: stride 3 unsupported', [wp], 'pack with stride 3')

    dx = nan(1, 12, 12, 16)
    refused([ops.rec_conv_dgrad(val(1, 4, 4, 16), val(4096).flatten(), dx, 3, 3, 3, 1)], 'conv_dgrad: stride 3 unsupported', [dx], 'data gradient with stride 3')

    if dtype == BF16:                               # fp32 moves vectors of 4 channels: C = 12 is served there
        y = nan(1, 4, 4, 8)
        refused([ops.rec_conv_fwd(val(1, 4, 4, 12), val(4096).flatten(), y, 8, 1, 1, 1, 0)], 'C=12 must be a multiple of 8', [y], 'C = 12 in bf16')

    # a weight gradient with ragged K: the callers pad dy with zero channels instead (test_zero_padded_k_in_the_backward)
    dy = val(2, 20, 20, 32)[..., :27]
    ga = nan(27, 64, 1, 1, dt=torch.float32)
    ws = nan(ops.wgrad_ws_bytes(2, 20, 20, 64, 32, 1, 1, 1, 0, dtype) // 4 + 1, dt=torch.float32)
    refused([ops.rec_conv_wgrad(val(2, 20, 20, 64), dy, ga, None, 1, 1, 1, 0, ws)], 'K=27 must be multiples of', [ga, ws], 'weight gradient with K = 27')

    # a residual pitch below K (the tensor-level wrapper cannot state one: the record's pitch is lowered by hand)
    y = nan(1, 4, 4, 16)
    rec = ops.rec_conv_fwd(val(1, 4, 4, 16), val(4096).flatten(), y, 16, 1, 1, 1, 0, res=val(1, 4, 4, 16))
    args = list(rec[1])
    assert args[6] == 16, 'hdy_conv_fwd: the residual pitch is no longer the seventh argument'
    args[6] = 15
    refused([(rec[0], tuple(args)) + tuple(rec[2:])], 'residual pitch 15 < K', [y], 'residual pitch below K')

    # 7x7: 49 taps against the 31 tap bits of the generic kernel's loader (5x5 = 25 is the largest square window served)
    e = X.reference(X.REFUSED_WINDOW_CASE)
    X.check_preconditions(e)
    L = Layer(e, dtype)
    y = nan(e.case[0], e.Ho, e.Wo, e.case[4])
    refused([ops.rec_conv_fwd(L.xd, L.wp, y, *L.geo)], "7 x 7 tap window beyond the loader's 31 tap bits", [y], '7x7 forward')
