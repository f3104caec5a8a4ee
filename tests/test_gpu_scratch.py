"""Poison-scratch invariance, repeat determinism and direct reference tests for the kernel entry points (MI355X).

Every parity test elsewhere runs a kernel once, on fresh allocations whose contents are whatever the caching allocator left there.  A kernel
that reads memory it did not write, or that races, can pass them.  Here each row is one code path of one entry point (the table below); its
call is run on identical inputs three times, and before every run each buffer the call only writes or uses as scratch (workspaces, statistic
slabs, outputs written with accumulate = 0, and one spare slab behind every slab array) is filled with a different byte pattern:

    A  zero bytes
    B  all-ones bytes: NaN in fp32, bf16 and fp64, and it survives a multiplication by zero
    C  a huge finite value (0x7F7F7F7F fp32, 0x7F7F bf16, 0x7F7F7F7F7F7F7F7F fp64): survives max / min / clamps, which drop NaN

The outputs must be bit-identical across A, B and C (compared as integer views), the pitch lanes of an output's allocation outside its
channel slice (and every spare slab) must still hold the pattern, the output must match a plain fp32 / fp64 CPU reference once, and the
kernel family the row is about must appear in the dispatch log (entry points that note no dispatch name instead assert the host-side query
that picks their path).  Read-write operands (running statistics, the input slabs) are restored before every run.

Safety rule: a buffer that holds indices, counts, list heads or links is never filled with an arbitrary bit pattern — a buggy kernel could
turn one into an address.  None of the rows below owns such a buffer.

Not covered here: hdy_nms_batched, hdy_mask_select's scratch and a whole training step with every non-zeroed plan buffer poisoned.  Those need
in-range fills of their index buffers and are separate work.  The fused detection loss (hdy_det_loss_ex, whose records carry links and list
heads) has its stale-workspace test in tests/test_gpu_loss_direct.py: a call after a larger one on the same, never zeroed, record region must
be bit-equal to a fresh call (stale records of a valid call hold in-range links, so nothing arbitrary is ever written into an index buffer).

Repeat determinism: each row is also run R times on the same operands with a launch of a different family running concurrently on a side
stream before every repeat (occupancy and timing change); every repeat must be bit-identical to the first.  The project promises fixed-order
reductions without atomics on this path.  Exempt, by design: roi_align backward (fp32 atomics in any order, roi.hip) and the fused loss
scalar (fp64 atomics over workgroup partials; its logits gradient must still be bit-identical, see tests/test_gpu_loss_forms.py).
"""
import fnmatch
from contextlib import ExitStack

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from hd_yolo_amd import _lib, ops  # noqa: E402
from test_gpu_kernels import DEV, TOL, assert_close, from_dev_nhwc, q, rnd, to_dev_nhwc  # noqa: E402

BF16, F32 = torch.bfloat16, torch.float32
INT_VIEW = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float64: torch.int64}
PATTERN = {'A': {torch.int32: 0, torch.int16: 0, torch.int64: 0},
           'B': {torch.int32: -1, torch.int16: -1, torch.int64: -1},
           'C': {torch.int32: 0x7F7F7F7F, torch.int16: 0x7F7F, torch.int64: 0x7F7F7F7F7F7F7F7F}}
REPEATS = 6


def bits(t):
    return t.contiguous().view(INT_VIEW[t.dtype]).clone()


class Case:
    """One call of one entry point: `recs` (launch records, built once: every pointer is fixed), the buffers it only writes (`buf`, poisoned
    whole before every run), its outputs (`out`: views into those buffers, compared bit for bit) and read-write operands (`inout`)."""

    def __init__(self, name, families=()):
        self.name, self.families = name, tuple(families)
        self.scratch, self.outs, self.resets, self.recs, self.check = [], [], [], [], None

    def buf(self, label, shape, dtype=torch.float32, workspace=False):
        t = torch.empty(shape, dtype=dtype, device=DEV)
        self.scratch.append((label, t, workspace))
        return t

    def out(self, label, view):
        self.outs.append((label, view))
        return view

    def inout(self, t, init):
        self.resets.append((t, init.clone()))
        return t


def fill(t, pat):
    t.view(INT_VIEW[t.dtype]).fill_(PATTERN[pat][INT_VIEW[t.dtype]])


def run_case(case, pat):
    for _, t, _ in case.scratch:
        fill(t, pat)
    for t, init in case.resets:
        t.copy_(init)
    _lib.dispatch_log(reset=True)
    ops.run(case.recs)
    torch.cuda.synchronize()
    return {label: bits(v) for label, v in case.outs}, _lib.dispatch_log(reset=True)


def check_untouched(case, pat):
    """lanes of an output's allocation that no output view covers (pitch lanes, spare slabs) still hold the pattern"""
    for label, base, workspace in case.scratch:
        views = [v for _, v in case.outs if v.untyped_storage().data_ptr() == base.untyped_storage().data_ptr()]
        if workspace or not views:
            continue                                  # a workspace: what else is left in it is not an output
        free = torch.ones(base.shape, dtype=torch.bool, device=DEV)
        for v in views:
            free.as_strided(v.shape, v.stride(), v.storage_offset() - base.storage_offset()).fill_(False)
        iv = base.view(INT_VIEW[base.dtype])
        bad = (iv[free] != PATTERN[pat][iv.dtype]).sum().item()
        assert bad == 0, f'{case.name}: {bad} elements of {label} outside its output view were written (pattern {pat})'


def assert_families(case, log):
    """every name pattern of the row (fnmatch: 'igemm_*') matches an entry of the dispatch log"""
    for fam in case.families:
        assert any(fnmatch.fnmatchcase(n, fam) for n in log), f'{case.name}: expected kernel family {fam} in the dispatch log, got {log}'


# ------------------------------------------------------------------------------------------------------------------------- row builders
def _conv_ref(x, w, stride, pad):
    return F.conv2d(x, w, None, stride, pad)


def conv_fwd_case(name, N, H, W, C, K, R, stride, pad, families, res=True, accumulate=False, band_cap=None):
    """forward with BatchNorm statistic slabs, and the eval epilogue (scale / shift / SiLU, the residual operand on stride 1), accumulate = 0;
    accumulate: the epilogue adds into an output that holds ones (conv_case's form; no residual).  band_cap: the filter-resident 3x3 kernel's
    persistent grid (768 at 32 channels, 512 at 64, conv3x3.hip conv3x3_grid) — the shape must leave a remainder of 8 x 16 tiles for the band split"""
    dt = BF16
    if band_cap is not None:
        tiles = N * (H // 8) * (W // 16)
        assert ops.stat_slabs(N, H, W, C, K, R, R, stride, pad, dt) == band_cap < tiles and tiles % band_cap, (tiles, band_cap)
    c = Case(name, families)
    x = q(rnd((N, C, H, W), 1), dt)
    w = rnd((K, C, R, R), 2, (3.0 / (C * R * R)) ** 0.5)
    xd = to_dev_nhwc(x, dt, ld=C + 8, off=8)
    wp = ops.pack_alloc(K, C, R, R, stride, pad, ops.PACK_FWD, dt, DEV)
    ops.run([ops.rec_pack(w.to(DEV), None, stride, pad, ops.PACK_FWD, wp)])
    Ho, Wo = ops.out_dim(H, R, stride, pad), ops.out_dim(W, R, stride, pad)
    mt = ops.stat_slabs(N, H, W, C, K, R, R, stride, pad, dt)
    y = c.out('y', c.buf('y', (N, Ho, Wo, K + 8), dt)[..., 8:])
    st = c.out('stats', c.buf('stats', (mt + 1, 2, K))[:mt])                 # + one spare slab: nothing may write it
    sc, sh = rnd((K,), 3).abs() + 0.5, rnd((K,), 4)
    rs = q(rnd((N, K, Ho, Wo), 5), dt) if res and stride == 1 and not accumulate else None
    y2 = c.out('y_eval', c.buf('y_eval', (N, Ho, Wo, K + 8), dt)[..., :K])
    if accumulate:
        c.inout(y2, torch.ones(y2.shape, dtype=dt, device=DEV))
    c.recs = [ops.rec_conv_fwd(xd, wp, y, K, R, R, stride, pad, stats=st),
              ops.rec_conv_fwd(xd, wp, y2, K, R, R, stride, pad, scale=sc.to(DEV), shift=sh.to(DEV), act=ops.ACT_SILU, accumulate=accumulate,
                               res=None if rs is None else to_dev_nhwc(rs, dt, ld=K + 16, off=16))]

    def check():
        ref = _conv_ref(x, q(w, dt), stride, pad)
        assert_close(from_dev_nhwc(y), ref, TOL[dt], f'{name} forward')
        s = st.sum(0).cpu()
        assert_close(s[0], ref.sum((0, 2, 3)), 1e-3, f'{name} statistics sum')
        assert_close(s[1], (ref * ref).sum((0, 2, 3)), 1e-3, f'{name} statistics sum of squares')
        ref2 = F.silu(ref * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)) + (0 if rs is None else rs) + (1.0 if accumulate else 0.0)
        assert_close(from_dev_nhwc(y2), ref2, TOL[dt] * 2, f'{name} eval epilogue')
    c.check = check
    return c


def stem_fwd_case(name, N, H, W, K, families):
    dt = BF16
    c = Case(name, families)
    img = q(rnd((N, 3, H, W), 1).abs(), dt)
    w = rnd((K, 3, 6, 6), 2, 0.2)
    prep = torch.empty((N, H + 4, W + 4, 4), dtype=dt, device=DEV)
    wp = ops.pack_alloc(K, 3, 6, 6, 2, 2, ops.PACK_STEM, dt, DEV)
    ops.run([ops.rec_stem_prep(img.to(DEV), prep), ops.rec_pack(w.to(DEV), None, 2, 2, ops.PACK_STEM, wp)])
    Ho, Wo = H // 2, W // 2
    mt = ops.stat_slabs(N, H, W, 3, K, 6, 6, 2, 2, dt)
    y = c.out('y', c.buf('y', (N, Ho, Wo, K), dt))
    st = c.out('stats', c.buf('stats', (mt + 1, 2, K))[:mt])
    sc, sh = rnd((K,), 5).abs() + 0.5, rnd((K,), 6)
    y2 = c.out('y_eval', c.buf('y_eval', (N, Ho, Wo, K), dt))
    c.recs = [ops.rec_conv_fwd(prep, wp, y, K, 6, 6, 2, 2, stats=st, stem_hw=(H, W)),
              ops.rec_conv_fwd(prep, wp, y2, K, 6, 6, 2, 2, scale=sc.to(DEV), shift=sh.to(DEV), act=ops.ACT_SILU, stem_hw=(H, W))]

    def check():
        ref = _conv_ref(img, q(w, dt), 2, 2)
        assert_close(from_dev_nhwc(y), ref, TOL[dt], f'{name} forward')
        s = st.sum(0).cpu()
        assert_close(s[0], ref.sum((0, 2, 3)), 1e-3, f'{name} statistics sum')
        assert_close(s[1], (ref * ref).sum((0, 2, 3)), 1e-3, f'{name} statistics sum of squares')
        assert_close(from_dev_nhwc(y2), F.silu(ref * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)), TOL[dt], f'{name} eval epilogue')
    c.check = check
    return c


def _dsilu(u):
    s = torch.sigmoid(u)
    return s * (1 + u * (1 - s))


def dgrad_case(name, N, H, W, C, K, R, stride, pad, families, stats=False, accumulate=False):
    """data gradient written with accumulate = 0 (accumulate: added to ones, conv_case's form); stats: two BatchNorm units' producer-side slabs
    over the halves of dx"""
    dt = BF16
    c = Case(name, families)
    Ho, Wo = ops.out_dim(H, R, stride, pad), ops.out_dim(W, R, stride, pad)
    dy = q(rnd((N, K, Ho, Wo), 5), dt)
    dyd = to_dev_nhwc(dy, dt, ld=K + 8, off=0)
    w = rnd((K, C, R, R), 2, (3.0 / (C * R * R)) ** 0.5)
    wpd = ops.pack_alloc(K, C, R, R, stride, pad, ops.PACK_DGRAD, dt, DEV)
    ops.run([ops.rec_pack(w.to(DEV), None, stride, pad, ops.PACK_DGRAD, wpd)])
    dx = c.out('dx', c.buf('dx', (N, H, W, C + 8), dt)[..., 8:])
    if accumulate:
        c.inout(dx, torch.ones(dx.shape, dtype=dt, device=DEV))
    reqs, units = None, []
    if stats:
        nslabs = ops.conv_dgrad_stat_slabs(N, H, W, C, K, R, R, stride, pad, dt)
        assert nslabs > 0
        for i, (c0, c1) in enumerate([(0, C // 2), (C // 2, C)]):
            yv = q(rnd((N, c1 - c0, H, W), 10 + i, 2.0), dt)
            sc, sh = (rnd((c1 - c0,), 30 + i).abs() + 0.5), rnd((c1 - c0,), 40 + i, 0.3)
            slabs = c.out(f'slabs{i}', c.buf(f'slabs{i}', (nslabs + 1, 2, c1 - c0))[:nslabs])
            units.append((c0, c1, yv, sc, sh, slabs))
        reqs = [ops.StatRequest(to_dev_nhwc(yv, dt), sc.to(DEV), sh.to(DEV), slabs, c0, ops.ACT_SILU) for c0, c1, yv, sc, sh, slabs in units]
    c.recs = [ops.rec_conv_dgrad(dyd, wpd, dx, R, R, stride, pad, accumulate=accumulate, stats=reqs)]

    def check():
        xr = torch.zeros((N, C, H, W), requires_grad=True)
        F.conv2d(xr, q(w, dt), None, stride, pad).backward(dy)
        got = from_dev_nhwc(dx)
        assert_close(got, xr.grad + (1.0 if accumulate else 0.0), TOL[dt] * 2, f'{name} data gradient')
        for c0, c1, yv, sc, sh, slabs in units:
            du = got[:, c0:c1].double() * _dsilu(yv.double() * sc.view(1, -1, 1, 1).double() + sh.view(1, -1, 1, 1).double())
            s = slabs.sum(0).cpu()
            assert_close(s[0], du.sum((0, 2, 3)).float(), 2e-2, f'{name} slab SUM du', elementwise=False)
            assert_close(s[1], (du * yv.double()).sum((0, 2, 3)).float(), 2e-2, f'{name} slab SUM du*y', elementwise=False)
    c.check = check
    return c


def wgrad_case(name, N, H, W, C, K, R, stride, pad, families, unaligned=False, dtype=BF16, accumulate=False, splits=None):
    """weight gradient, stacked grad_a / grad_b, accumulate = 0 (accumulate: added to 0 and 2, conv_case's form); unaligned: grad_a one float
    off 16 bytes (the scalar reduce kernel); splits: the generic kernel's pixel splits (the workspace holds one K x Q slab per split)"""
    dt = dtype
    if splits is not None:
        assert ops.wgrad_ws_bytes(N, H, W, C, K, R, R, stride, pad, dt) == splits * K * R * R * C * 4
    c = Case(name, families)
    x = q(rnd((N, C, H, W), 1), dt)
    Ho, Wo = ops.out_dim(H, R, stride, pad), ops.out_dim(W, R, stride, pad)
    dy = q(rnd((N, K, Ho, Wo), 5), dt)
    xd, dyd = to_dev_nhwc(x, dt, ld=C + 8, off=8), to_dev_nhwc(dy, dt, ld=K + 8, off=0)
    ws = c.buf('workspace', (ops.wgrad_ws_bytes(N, H, W, C, K, R, R, stride, pad, dt) // 4 + 1,))
    ka = K // 2
    if unaligned:
        ga = c.out('grad_a', c.buf('grad_a', (ka * C * R * R + 1,))[1:].view(ka, C, R, R))
    else:
        ga = c.out('grad_a', c.buf('grad_a', (ka, C, R, R)))
    gb = c.out('grad_b', c.buf('grad_b', (K - ka, C, R, R)))
    if accumulate:
        c.inout(ga, torch.zeros(ga.shape, device=DEV))
        c.inout(gb, torch.full(gb.shape, 2.0, device=DEV))
    c.recs = [ops.rec_conv_wgrad(xd, dyd, ga, gb, R, R, stride, pad, ws, accumulate=accumulate)]

    def check():
        wr = q(rnd((K, C, R, R), 2), dt).requires_grad_(True)
        F.conv2d(x, wr, None, stride, pad).backward(dy)
        g = torch.cat([ga.cpu(), gb.cpu() - (2.0 if accumulate else 0.0)])
        assert_close(g, wr.grad, TOL[dt] * 3, f'{name} weight gradient')
    c.check = check
    return c


def wgrad_stem_case(name, N, H, W, K, fused):
    dt = BF16
    c = Case(name, ['wgrad_stem_fused' if fused else 'wgrad_stem'])
    img = q(rnd((N, 3, H, W), 1), dt)
    prep = torch.zeros((N, H + 4, W + 4, 4), dtype=dt, device=DEV)
    ops.run([ops.rec_stem_prep(img.to(DEV), prep)])
    Ho, Wo = H // 2, W // 2
    M = N * Ho * Wo
    ws = c.buf('workspace', (ops.wgrad_ws_bytes(N, H, W, 3, K, 6, 6, 2, 2, dt, stem=True) // 4 + 16,))
    g = c.out('grad', c.buf('grad', (K, 3, 6, 6)))
    if fused:
        assert ops.wgrad_stem_fused_ok(N, H, W, K, dt)
        y = rnd((N, Ho, Wo, K), 2).to(dt).to(DEV)
        dz = rnd((N, Ho, Wo, K), 3).to(dt).to(DEV)
        scale, shift = (rnd((K,), 4).abs() + 0.5).to(DEV), rnd((K,), 5).to(DEV)
        mean, invstd = rnd((K,), 6, 0.1).to(DEV), (rnd((K,), 7).abs() + 0.5).to(DEV)
        ws_bn = torch.empty(ops.bn_bwd_ws_floats(M, K), dtype=torch.float32, device=DEV)
        dyt = torch.empty_like(y)
        ops.run([ops.rec_bn_act_bwd(dz, y, scale, shift, mean, invstd, dyt, torch.zeros(K, device=DEV), torch.zeros(K, device=DEV), ws_bn)])
        c1, c2 = (t.clone() for t in ops.bn_bwd_coeffs(ws_bn, M, K))
        c.recs = [ops.rec_conv_wgrad_stem_fused(prep, dz, y, scale, shift, mean, invstd, c1, c2, (H, W), g, None, ws)]
        dyr = dyt.float().cpu().permute(0, 3, 1, 2)                          # the bf16 dy of the two-launch path: the same rounding point
    else:
        dyr = q(rnd((N, K, Ho, Wo), 3), dt)
        c.recs = [ops.rec_conv_wgrad(prep, to_dev_nhwc(dyr, dt), g, None, 6, 6, 2, 2, ws, stem_hw=(H, W))]

    def check():
        wr = torch.zeros((K, 3, 6, 6), requires_grad=True)
        F.conv2d(img, wr, None, 2, 2).backward(dyr)
        assert_close(g.cpu(), wr.grad, TOL[dt] * 3, f'{name} weight gradient')
    c.check = check
    return c


def pack_case(name, K, C, R, stride, pad, kind):
    """the packed weight buffer is the output: padding rows / columns must be written (as zeros) on every call"""
    dt = BF16
    c = Case(name, [{ops.PACK_FWD: 'pack_fwd', ops.PACK_DGRAD: 'pack_dgrad', ops.PACK_STEM: 'pack_stem'}[kind]])
    w = rnd((K, C, R, R), 2, (3.0 / (C * R * R)) ** 0.5)
    n = _lib.query('hdy_conv_pack_elems', K, C, R, R, stride, pad, kind, ops.dcode(dt))
    wp = c.out('packed', c.buf('packed', (n,), dt))
    assert n > K * C * R * R                          # the layout has padding the kernel must fill
    c.recs = [ops.rec_pack(w.to(DEV), None, stride, pad, kind, wp)]

    def check():                                      # the packed buffer drives its convolution
        N, H, W = 2, 12, 20
        if kind == ops.PACK_STEM:
            img = q(rnd((N, 3, H, W), 1).abs(), dt)
            prep = torch.empty((N, H + 4, W + 4, 4), dtype=dt, device=DEV)
            y = torch.empty((N, H // 2, W // 2, K), dtype=dt, device=DEV)
            ops.run([ops.rec_stem_prep(img.to(DEV), prep), ops.rec_conv_fwd(prep, wp, y, K, 6, 6, 2, 2, stem_hw=(H, W))])
            assert_close(from_dev_nhwc(y), _conv_ref(img, q(w, dt), 2, 2), TOL[dt], f'{name} through the stem convolution')
            return
        Ho, Wo = ops.out_dim(H, R, stride, pad), ops.out_dim(W, R, stride, pad)
        if kind == ops.PACK_FWD:
            x = q(rnd((N, C, H, W), 1), dt)
            y = torch.empty((N, Ho, Wo, K), dtype=dt, device=DEV)
            ops.run([ops.rec_conv_fwd(to_dev_nhwc(x, dt), wp, y, K, R, R, stride, pad)])
            assert_close(from_dev_nhwc(y), _conv_ref(x, q(w, dt), stride, pad), TOL[dt], f'{name} through the forward convolution')
        else:
            dy = q(rnd((N, K, Ho, Wo), 5), dt)
            dx = torch.empty((N, H, W, C), dtype=dt, device=DEV)
            ops.run([ops.rec_conv_dgrad(to_dev_nhwc(dy, dt), wp, dx, R, R, stride, pad)])
            xr = torch.zeros((N, C, H, W), requires_grad=True)
            F.conv2d(xr, q(w, dt), None, stride, pad).backward(dy)
            assert_close(from_dev_nhwc(dx), xr.grad, TOL[dt] * 2, f'{name} through the data gradient')
    c.check = check
    return c


def fused_1x1_case(name, K, Nb, Wd, pair, stats=False):
    """hdy_conv1x1_bwd_fused after the statistics-only BatchNorm backward: the BatchNorm workspace, the fused workspace, dx (accumulate = 0),
    the stacked weight gradients and (stats) two units' producer-side slabs"""
    dt = BF16
    C, M = K, Nb * Wd
    c = Case(name, ['conv1x1_bwd_%d' % K, 'bn_bwd_reduce4'])
    flat = lambda t: t.permute(0, 2, 3, 1).reshape(M, t.shape[1]).double()
    dz = q(rnd((Nb, K, 1, Wd), 1), dt)
    y = q(rnd((Nb, K, 1, Wd), 2, 2.0) + rnd((1, K, 1, 1), 3), dt)
    x = q(rnd((Nb, C, 1, Wd), 4), dt)
    w = rnd((K, C, 1, 1), 5, 0.3)
    gamma, beta = rnd((K,), 7) + 1.5, rnd((K,), 8, 0.3)
    Ka = K // 2 if pair else K
    dz_a = to_dev_nhwc(dz[:, :Ka], dt, ld=Ka + 16, off=8)
    dz_b = to_dev_nhwc(dz[:, Ka:], dt, ld=K + 8, off=0) if pair else None
    yd, xd = to_dev_nhwc(y, dt), to_dev_nhwc(x, dt, ld=C + 24, off=16)
    yq = flat(y)
    mean, var = yq.mean(0), yq.var(0, unbiased=False)
    invstd = 1.0 / torch.sqrt(var + 1e-3)
    scale, shift = gamma.double() * invstd, beta.double() - mean * gamma.double() * invstd
    dev = lambda t: t.float().contiguous().to(DEV)
    sc_d, sh_d, mu_d, is_d = dev(scale), dev(shift), dev(mean), dev(invstd)
    wpd = ops.pack_alloc(K, C, 1, 1, 1, 0, ops.PACK_DGRAD, dt, DEV)
    ops.run([ops.rec_pack(w.to(DEV), None, 1, 0, ops.PACK_DGRAD, wpd)])
    ws = c.buf('bn_workspace', (ops.bn_bwd_ws_floats(M, K),), workspace=True)
    dg = c.out('dgamma', c.buf('dgamma', (K,)))
    db = c.out('dbeta', c.buf('dbeta', (K,)))
    c1_d, c2_d = ops.bn_bwd_coeffs(ws, M, K)
    c.out('c1', c1_d)
    c.out('c2', c2_d)
    f1ws = c.buf('fused_workspace', (ops.fused_1x1_ws_bytes(M, C, K) // 4 + 16,))
    dx = c.out('dx', c.buf('dx', (Nb, 1, Wd, C + 8), dt)[..., 8:])
    gw = c.buf('grad', (K, C, 1, 1))
    ga, gb = c.out('grad_a', gw[:Ka]), (c.out('grad_b', gw[Ka:]) if pair else None)
    units, reqs = [], None
    if stats:
        nslabs = ops.fused_1x1_stat_slabs(M, C, K, dt)
        assert nslabs > 0
        for i, (u0, u1) in enumerate([(0, C // 2), (C // 2, C)]):
            uy = q(rnd((Nb, u1 - u0, 1, Wd), 10 + i, 2.0), dt)
            usc, ush = rnd((u1 - u0,), 30 + i).abs() + 0.5, rnd((u1 - u0,), 40 + i, 0.3)
            slabs = c.out(f'slabs{i}', c.buf(f'slabs{i}', (nslabs + 1, 2, u1 - u0))[:nslabs])
            units.append((u0, u1, uy, usc, ush, slabs))
        reqs = [ops.StatRequest(to_dev_nhwc(uy, dt), usc.to(DEV), ush.to(DEV), slabs, u0, ops.ACT_SILU) for u0, u1, uy, usc, ush, slabs in units]
    if pair:
        bn_rec = ops.rec_bn_act_bwd_pair(dz_a, dz_b, yd, sc_d, sh_d, mu_d, is_d, None, dg[:Ka], db[:Ka], dg[Ka:], db[Ka:], ws)
    else:
        bn_rec = ops.rec_bn_act_bwd(dz_a, yd, sc_d, sh_d, mu_d, is_d, None, dg, db, ws)
    c.recs = [bn_rec, ops.rec_conv1x1_bwd_fused(dz_a, dz_b, yd, sc_d, sh_d, mu_d, is_d, c1_d, c2_d, xd, wpd, dx, ga, gb, f1ws, stats=reqs)]

    def check():
        u = yq * scale + shift
        du = flat(dz) * _dsilu(u)
        xh = (yq - mean) * invstd
        r1, r2 = du.mean(0), (du * xh).mean(0)
        assert_close(c1_d.cpu(), r1.float(), 2e-3, f'{name} c1')
        assert_close(db.cpu(), du.sum(0).float(), 2e-3, f'{name} dbeta')
        assert_close(dg.cpu(), (du * xh).sum(0).float(), 2e-3, f'{name} dgamma')
        dyr = (scale * (du - r1 - xh * r2)).float().to(dt).double()
        got_dx = dx.float().cpu().reshape(M, C)
        assert_close(got_dx, (dyr @ q(w, dt)[:, :, 0, 0].double()).float(), 1.5e-2, f'{name} dx')
        assert_close(gw.cpu()[:, :, 0, 0], (dyr.T @ flat(x)).float(), 1.5e-2, f'{name} dW')
        for u0, u1, uy, usc, ush, slabs in units:
            udu = got_dx[:, u0:u1].double() * _dsilu(flat(uy) * usc.double() + ush.double())
            s = slabs.sum(0).cpu()
            assert_close(s[0], udu.sum(0).float(), 2e-2, f'{name} slab SUM du', elementwise=False)
            assert_close(s[1], (udu * flat(uy)).sum(0).float(), 2e-2, f'{name} slab SUM du*y', elementwise=False)
    c.check = check
    return c


def _bn_params(K, seed):
    gamma, beta = rnd((K,), seed).abs() + 0.5, rnd((K,), seed + 1) * 0.3
    rm, rv = rnd((K,), seed + 2) * 0.1, rnd((K,), seed + 3).abs() + 0.5
    return gamma, beta, rm, rv


def bn_finalize_case(name, mt, K, Ka=None):
    """hdy_bn_finalize[_pair] on mt slabs (two stages with their fp64 workspace above 1024); the slab array has one spare slab that no kernel
    writes: a finalize that reads past mt sees the pattern"""
    c = Case(name, ['bn_finalize_2stage' if mt > 1024 else 'bn_finalize'])
    count = mt * 100
    g = torch.Generator().manual_seed(mt + K)
    data = torch.stack([torch.randn((mt, K), generator=g) * 10, torch.rand((mt, K), generator=g) * 100 + 60], 1)
    sbase = c.buf('stats', (mt + 1, 2, K))
    c.inout(sbase[:mt], data)
    gamma, beta, rm, rv = _bn_params(K, 3)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    rmd, rvd = c.inout(torch.empty(K, device=DEV), rm), c.inout(torch.empty(K, device=DEV), rv)
    c.out('running_mean', rmd)
    c.out('running_var', rvd)
    scale, shift, mean, inv = (c.out(n, c.buf(n, (K,))) for n in ('scale', 'shift', 'save_mean', 'save_invstd'))
    wsb = _lib.query('hdy_bn_finalize_workspace_bytes', mt, K)
    assert (wsb > 0) == (mt > 1024)
    ws = c.buf('workspace', (wsb // 8,), torch.float64) if wsb else None
    st = sbase[:mt]
    if Ka is None:
        c.recs = [ops.rec_bn_finalize(st, mt, K, count, gd, bd, rmd, rvd, scale, shift, mean, inv, ws=ws)]
    else:
        c.recs = [ops.rec_bn_finalize_pair(st, mt, K, Ka, count, (gd[:Ka], bd[:Ka], rmd[:Ka], rvd[:Ka]), (gd[Ka:], bd[Ka:], rmd[Ka:], rvd[Ka:]),
                                           scale, shift, mean, inv, ws=ws)]

    def check():
        s = data.double().sum(0)
        mu = s[0] / count
        var = s[1] / count - mu * mu
        isd = 1.0 / torch.sqrt(var + ops.BN_EPS)
        m = ops.BN_MOMENTUM
        for got, want, what in ((mean, mu, 'mean'), (inv, isd, 'invstd'), (scale, gamma.double() * isd, 'scale'),
                                (shift, beta.double() - mu * gamma.double() * isd, 'shift'), (rmd, (1 - m) * rm.double() + m * mu, 'running_mean'),
                                (rvd, (1 - m) * rv.double() + m * var * count / (count - 1), 'running_var')):
            assert_close(got.cpu(), want.float(), 1e-5, f'{name} {what}')
    c.check = check
    return c


def _bn_bwd_operands(M, K, dt, seed=1):
    dz = q(rnd((1, K, 1, M), seed), dt)
    y = q(rnd((1, K, 1, M), seed + 1, 2.0) + rnd((1, K, 1, 1), seed + 2), dt)
    scale, shift = rnd((K,), seed + 3).abs() + 0.5, rnd((K,), seed + 4)
    mean, invstd = rnd((K,), seed + 5, 0.3), rnd((K,), seed + 6).abs() + 0.5
    return dz, y, scale, shift, mean, invstd


def _bn_bwd_ref(dz, y, scale, shift, mean, invstd):
    """fp64 (du, xhat) of z = SiLU(scale * y + shift), flattened to (M, K)"""
    fl = lambda t: t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).double()
    yv = fl(y)
    du = fl(dz) * _dsilu(yv * scale.double() + shift.double())
    return du, (yv - mean.double()) * invstd.double()


def bn_act_bwd_case(name, M, K, dt, blocks, reduce):
    """hdy_bn_act_bwd (reduce over hdy_bn_bwd_blocks(M) row blocks -> finalize -> apply): dy, dgamma / dbeta (accumulate = 0), c1 / c2; reduce:
    the reduce kernel's dispatch name (bn_bwd_reduce4: bf16, four channels per lane; bn_bwd_reduce: the generic one); 1024 row blocks and more take
    the wide finalize instance"""
    assert ops.bn_bwd_blocks(M) == blocks
    c = Case(name, [reduce, 'bn_bwd_finalize_wide' if blocks >= 1024 else 'bn_bwd_finalize'])
    dz, y, scale, shift, mean, invstd = _bn_bwd_operands(M, K, dt)
    ws = c.buf('workspace', (ops.bn_bwd_ws_floats(M, K),), workspace=True)
    dy = c.out('dy', c.buf('dy', (1, 1, M, K + 8), dt)[..., 8:])
    dg, db = c.out('dgamma', c.buf('dgamma', (K,))), c.out('dbeta', c.buf('dbeta', (K,)))
    c1, c2 = ops.bn_bwd_coeffs(ws, M, K)
    c.out('c1', c1)
    c.out('c2', c2)
    d = lambda t: t.to(DEV)
    c.recs = [ops.rec_bn_act_bwd(to_dev_nhwc(dz, dt, ld=K + 8, off=0), to_dev_nhwc(y, dt), d(scale), d(shift), d(mean), d(invstd), dy, dg, db, ws)]

    def check():
        du, xh = _bn_bwd_ref(dz, y, scale, shift, mean, invstd)
        r1, r2 = du.mean(0), (du * xh).mean(0)
        tol = 1e-4 if dt == F32 else 2e-3
        assert_close(db.cpu(), du.sum(0).float(), tol, f'{name} dbeta')
        assert_close(dg.cpu(), (du * xh).sum(0).float(), tol, f'{name} dgamma')
        assert_close(c1.cpu(), r1.float(), tol, f'{name} c1')
        assert_close(c2.cpu(), r2.float(), tol, f'{name} c2')
        ref = scale.double() * (du - r1 - xh * r2)
        assert_close(dy.float().cpu().reshape(M, K), ref.float(), TOL[dt] * 3, f'{name} dy')
    c.check = check
    return c


def bn_bwd_finalize_slabs_case(name, n, K):
    c = Case(name, ['bn_bwd_finalize_wide' if n >= 1024 else 'bn_bwd_finalize'])
    count = n * 64
    g = torch.Generator().manual_seed(n)
    data = torch.randn((n, 2, K), generator=g) * 8
    sbase = c.buf('slabs', (n + 1, 2, K))
    c.inout(sbase[:n], data)
    mean, invstd = rnd((K,), 5, 0.3), rnd((K,), 6).abs() + 0.5
    dg, db, c1, c2 = (c.out(nm, c.buf(nm, (K,))) for nm in ('dgamma', 'dbeta', 'c1', 'c2'))
    c.recs = [ops.rec_bn_bwd_finalize_slabs(sbase[:n], count, mean.to(DEV), invstd.to(DEV), dg, db, c1, c2)]

    def check():
        s = data.double().sum(0)
        dgr = invstd.double() * (s[1] - mean.double() * s[0])
        for got, want, what in ((db, s[0], 'dbeta'), (dg, dgr, 'dgamma'), (c1, s[0] / count, 'c1'), (c2, dgr / count, 'c2')):
            assert_close(got.cpu(), want.float(), 1e-5, f'{name} {what}')
    c.check = check
    return c


def colsum_case(name, M, K, dt, blocks):
    assert ops.bn_bwd_blocks(M) == blocks
    c = Case(name, ['bn_bwd_reduce', 'bn_bwd_finalize_wide' if blocks >= 1024 else 'bn_bwd_finalize'])
    dz = q(rnd((1, K, 1, M), 3), dt)
    ws = c.buf('workspace', (ops.bn_bwd_ws_floats(M, K),))             # what ops.rec_colsum asks for (>= hdy_colsum_workspace_bytes)
    out = c.out('out', c.buf('out', (K,)))
    c.recs = [ops.rec_colsum(to_dev_nhwc(dz, dt, ld=K + 8, off=8), out, ws)]
    c.check = lambda: assert_close(out.cpu(), dz.double().sum((0, 2, 3)).float(), 1e-5, f'{name} column sums')
    return c


def _raw(name, args, keep):
    """a launch record for an entry point that ops.py wraps with its own allocations: our buffers instead"""
    return (name, args, tuple(keep))


def groupnorm_case(name, N, H, W, C, G, dt, backward):
    """hdy_groupnorm_fwd (y, statistics, coefficients, workspace) or hdy_groupnorm_bwd (dx, dgamma / dbeta with accumulate = 0, coefficient
    scratch, workspace) of ReLU(GroupNorm(x)); x a channel slice of a wider buffer"""
    c = Case(name, ['groupnorm_bwd' if backward else 'groupnorm_fwd'])
    x = (rnd((N, H, W, C), 1, 2.0) + rnd((1, 1, 1, C), 2)).to(dt)
    gamma, beta = rnd((C,), 3) + 1.2, rnd((C,), 4, 0.4)
    dout = rnd((N, H, W, C), 5).to(dt)
    xd = torch.full((N, H, W, C + 16), 3.0, dtype=dt, device=DEV)[..., 8:8 + C]
    xd.copy_(x)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    wsf = _lib.query('hdy_groupnorm_workspace_floats', N, C)
    xr = x.float().permute(0, 3, 1, 2).clone().requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    ref = F.relu(F.group_norm(xr, G, gr, br, 1e-5))
    ref.backward(dout.float().permute(0, 3, 1, 2))
    if not backward:
        y = c.out('y', c.buf('y', (N, H, W, C + 8), dt)[..., :C])
        stat, ab = c.out('stat', c.buf('stat', (N, G, 2))), c.out('ab', c.buf('ab', (N, 2, C)))
        ws = c.buf('workspace', (wsf,))
        c.recs = [_raw('hdy_groupnorm_fwd', (xd.data_ptr(), C + 16, gd.data_ptr(), bd.data_ptr(), y.data_ptr(), C + 8, stat.data_ptr(), ab.data_ptr(),
                                             N, H * W, C, G, 1e-5, 1, ops.dcode(dt), ws.data_ptr(), wsf), (xd, gd, bd, y, stat, ab, ws))]
        c.check = lambda: assert_close(y.float().cpu(), ref.detach().permute(0, 2, 3, 1), TOL[dt], f'{name} y', elementwise=False)
        return c
    _, saved = ops.groupnorm_relu_fwd(xd, gd, bd, G)
    stat, ab = saved
    dod = dout.to(DEV)
    dx = c.out('dx', c.buf('dx', (N, H, W, C + 8), dt)[..., 8:])
    dg, db = c.out('dgamma', c.buf('dgamma', (C,))), c.out('dbeta', c.buf('dbeta', (C,)))
    coef = c.buf('coef', (N, 3, C), workspace=True)
    ws = c.buf('workspace', (wsf,))
    c.recs = [_raw('hdy_groupnorm_bwd', (dod.data_ptr(), C, xd.data_ptr(), C + 16, gd.data_ptr(), stat.data_ptr(), ab.data_ptr(), dx.data_ptr(), C + 8,
                                         dg.data_ptr(), db.data_ptr(), 0, coef.data_ptr(), N, H * W, C, G, 1, ops.dcode(dt), ws.data_ptr(), wsf),
                   (dod, xd, gd, stat, ab, dx, dg, db, coef, ws))]

    def check():
        assert_close(dx.float().cpu(), xr.grad.permute(0, 2, 3, 1), TOL[dt], f'{name} dx', elementwise=False)
        assert_close(dg.cpu(), gr.grad, 2e-3, f'{name} dgamma', elementwise=False)
        assert_close(db.cpu(), br.grad, 2e-3, f'{name} dbeta', elementwise=False)
    c.check = check
    return c


def softdice_case(name, N, H, W, nc):
    """hdy_softdice on 4-float pixels (<= 4 classes: the gradient is written for whole pixels, padding channels as zeros): loss, gradient, workspace"""
    from oracle import seg_ref
    c = Case(name, ['softdice'])
    ld = 4
    logits = rnd((N, H, W, ld), 11, 3.0)
    logits[..., nc:] = 0
    lab = torch.randint(0, max(nc, 2), (N, H, W), generator=torch.Generator().manual_seed(12))
    masks = F.one_hot(lab, max(nc, 2)).permute(0, 3, 1, 2).float()[:, :nc].contiguous()
    ld_d, md, up = logits.to(DEV), masks.to(DEV), torch.tensor([1.7], device=DEV)
    wsf = _lib.query('hdy_softdice_workspace_floats', N, nc)
    loss = c.out('loss', c.buf('loss', (1,)))
    dl = c.out('dlogits', c.buf('dlogits', (N, H, W, ld)))
    ws = c.buf('workspace', (wsf,))
    c.recs = [_raw('hdy_softdice', (ld_d.data_ptr(), ld, md.data_ptr(), None, N, H * W, nc, loss.data_ptr(), up.data_ptr(), dl.data_ptr(), ld,
                                    ws.data_ptr(), wsf), (ld_d, md, up, loss, dl, ws))]

    def check():
        lr = logits[..., :nc].permute(0, 3, 1, 2).clone().requires_grad_(True)
        ref = 1 + seg_ref.soft_dice_criterion(torch.softmax(lr, 1), masks, None)
        (ref * 1.7).backward()
        assert abs(loss.item() - ref.item()) < 1e-5
        assert_close(dl.cpu()[..., :nc].permute(0, 3, 1, 2), lr.grad, 1e-4, f'{name} gradient', elementwise=False)
        assert dl[..., nc:].abs().max().item() == 0
    c.check = check
    return c


def sppf_case(name, N, H, W, C, dt, families):
    """hdy_sppf_pool_fwd (three levels into channel slices of one buffer, three position tables) followed by hdy_sppf_pool_bwd from those
    tables: the position tables are written before they are read, and hold tap numbers that are only compared, never used as an address"""
    c = Case(name, families)
    x = q(rnd((N, C, H, W), 1), dt)
    g = q(rnd((N, 4 * C, H, W), 2), dt)
    ld = 4 * C + 8
    xd = to_dev_nhwc(x, dt, ld=ld)
    cat = c.buf('cat', (N, H, W, ld), dt)
    ys = [c.out(f'y{i}', cat[..., i * C:(i + 1) * C]) for i in (1, 2, 3)]
    idx = [c.out(f'idx{i}', c.buf(f'idx{i}', (N, H, W, C // 4))) for i in (1, 2, 3)]          # four position bytes per fp32 word of the buffer
    gd = to_dev_nhwc(g, dt)
    gs = [gd[..., i * C:(i + 1) * C] for i in range(4)]
    dx = c.out('dx', c.buf('dx', (N, H, W, C + 8), dt)[..., 8:])
    c.recs = [ops.rec_sppf_pool_fwd(xd, ys[0], ys[1], ys[2], [t.view(torch.uint8) for t in idx]), ops.rec_sppf_pool_bwd(gs[0], gs[1], gs[2], gs[3], [t.view(torch.uint8) for t in idx], dx)]

    def check():
        xr = x.clone().requires_grad_(True)
        y1 = F.max_pool2d(xr, 5, 1, 2)
        y2 = F.max_pool2d(y1, 5, 1, 2)
        y3 = F.max_pool2d(y2, 5, 1, 2)
        torch.cat([xr, y1, y2, y3], 1).backward(g)
        for got, want in zip(ys, (y1, y2, y3)):
            assert torch.equal(from_dev_nhwc(got), want.detach()), f'{name} forward'
        assert_close(from_dev_nhwc(dx), xr.grad, TOL[dt], f'{name} backward')
    c.check = check
    return c


def upsample_case(name, N, H, W, C, dt):
    """hdy_upsample2x_fwd and hdy_upsample2x_bwd with accumulate = 0 (the upsample kernels note no dispatch name), pitched outputs"""
    c = Case(name)
    x, g = q(rnd((N, C, H, W), 1), dt), q(rnd((N, C, 2 * H, 2 * W), 2), dt)
    y = c.out('y', c.buf('y', (N, 2 * H, 2 * W, C + 8), dt)[..., 8:])
    dx = c.out('dx', c.buf('dx', (N, H, W, C + 8), dt)[..., :C])
    c.recs = [ops.rec_upsample_fwd(to_dev_nhwc(x, dt, ld=C + 8, off=8), y), ops.rec_upsample_bwd(to_dev_nhwc(g, dt), dx, accumulate=False)]

    def check():
        assert torch.equal(from_dev_nhwc(y), F.interpolate(x, scale_factor=2.0, mode='nearest')), f'{name} forward'
        assert_close(from_dev_nhwc(dx), g.view(N, C, H, 2, W, 2).sum((3, 5)), TOL[dt], f'{name} backward')
    c.check = check
    return c


# ------------------------------------------------------------------------------------------------------------------------------ the table
D0 = {'HDY_DEEP_MIN_TILES': 1}
ROWS = [
    # (id, options, builder); families are fnmatch patterns over the dispatch log
    ('pack_fwd-K40C24-3x3', {}, lambda: pack_case('hdy_conv_pack PACK_FWD', 40, 24, 3, 1, 1, ops.PACK_FWD)),
    ('pack_fwd-K136C64-1x1', {}, lambda: pack_case('hdy_conv_pack PACK_FWD', 136, 64, 1, 1, 0, ops.PACK_FWD)),
    ('pack_dgrad-s1-K24C40', {}, lambda: pack_case('hdy_conv_pack PACK_DGRAD stride 1', 24, 40, 3, 1, 1, ops.PACK_DGRAD)),
    ('pack_dgrad-s2-K48C24', {}, lambda: pack_case('hdy_conv_pack PACK_DGRAD stride 2', 48, 24, 3, 2, 1, ops.PACK_DGRAD)),
    ('pack_stem-K24', {}, lambda: pack_case('hdy_conv_pack PACK_STEM', 24, 3, 6, 2, 2, ops.PACK_STEM)),
    # forward with statistics + eval epilogue
    ('fwd-igemm_128x128x2', {}, lambda: conv_fwd_case('igemm_128x128x2 fwd', 2, 20, 20, 96, 96, 3, 1, 1, ['igemm_128x128x2*'])),
    ('fwd-igemm_128x64x2', {}, lambda: conv_fwd_case('igemm_128x64x2 fwd', 2, 20, 20, 48, 48, 1, 1, 0, ['igemm_128x64x2*'])),
    ('fwd-deep_256x128', {'HDY_NO_CONV3X3_C128': 1, **D0}, lambda: conv_fwd_case('deep_256x128 fwd', 3, 40, 40, 128, 128, 3, 1, 1, ['deep_256x128'])),
    ('fwd-deep_256x256', {'HDY_DEEP_BN': 256, **D0}, lambda: conv_fwd_case('deep_256x256 fwd', 3, 40, 40, 256, 256, 3, 1, 1, ['deep_256x128', 'deep_256x256'])),
    ('fwd-conv3x3_c32', {}, lambda: conv_fwd_case('conv3x3_c32 fwd', 2, 16, 32, 32, 32, 3, 1, 1, ['conv3x3_c32'])),
    ('fwd-conv3x3_c32-band', {}, lambda: conv_fwd_case('conv3x3_c32 fwd (band split)', 7, 128, 128, 32, 32, 3, 1, 1, ['conv3x3_c32'], band_cap=768)),
    ('fwd-conv3x3_c64', {}, lambda: conv_fwd_case('conv3x3_c64 fwd', 2, 16, 32, 64, 64, 3, 1, 1, ['conv3x3_c64'])),
    ('fwd-conv3x3_c64-band', {}, lambda: conv_fwd_case('conv3x3_c64 fwd (band split)', 5, 128, 128, 64, 64, 3, 1, 1, ['conv3x3_c64'], band_cap=512)),
    ('fwd-conv3x3_c128', {}, lambda: conv_fwd_case('conv3x3_c128 fwd', 3, 24, 40, 128, 128, 3, 1, 1, ['conv3x3_c128'])),
    ('fwd-conv3x3_c128-ragged', {}, lambda: conv_fwd_case('conv3x3_c128 fwd (ragged half)', 2, 16, 16, 128, 104, 3, 1, 1, ['conv3x3_c128'])),
    ('fwd-conv3x3s2_c32', {}, lambda: conv_fwd_case('conv3x3s2_c32 fwd', 2, 32, 64, 32, 64, 3, 2, 1, ['conv3x3s2_c32'])),
    ('fwd-conv3x3s2_c64', {}, lambda: conv_fwd_case('conv3x3s2_c64 fwd', 2, 32, 64, 64, 128, 3, 2, 1, ['conv3x3s2_c64'])),
    ('fwd-stem_patch', {}, lambda: stem_fwd_case('stem patch fwd', 3, 64, 192, 32, ['conv_stem'])),
    ('fwd-stem_generic', {'HDY_NO_STEM_KERNEL': 1}, lambda: stem_fwd_case('generic stem fwd', 2, 40, 56, 32, ['igemm_*'])),
    # data gradient (accumulate = 0), with and without producer-side statistics
    ('dgrad-igemm', {}, lambda: dgrad_case('igemm dgrad', 2, 20, 20, 64, 32, 1, 1, 0, ['igemm_*'])),
    ('dgrad-igemm-stats', {}, lambda: dgrad_case('igemm dgrad + statistics', 2, 24, 20, 64, 32, 1, 1, 0, ['igemm_*'], stats=True)),
    ('dgrad-igemm_walk', {}, lambda: dgrad_case('igemm stride-2 class walk', 2, 24, 24, 16, 32, 3, 2, 1, ['igemm_*_walk*'])),
    ('dgrad-conv3x3_c32', {}, lambda: dgrad_case('conv3x3_c32 dgrad', 2, 16, 32, 32, 32, 3, 1, 1, ['conv3x3_c32'])),
    ('dgrad-conv3x3_c64', {}, lambda: dgrad_case('conv3x3_c64 dgrad', 2, 16, 32, 64, 64, 3, 1, 1, ['conv3x3_c64'])),
    # producer-side statistics are served by the generic kernel only: their launch and hdy_conv_dgrad_stat_slabs both start the family walk at
    # CONV_IGEMM, so the patch-resident families (dgrad3x3s2 among them) are never asked; the stride-2 form is the generic kernel's class walk
    ('dgrad-igemm-stats-3x3', {}, lambda: dgrad_case('igemm 3x3 dgrad + statistics', 3, 16, 16, 32, 64, 3, 1, 1, ['igemm_*'], stats=True)),
    ('dgrad-igemm_walk-stats', {}, lambda: dgrad_case('igemm class walk + statistics', 5, 128, 128, 32, 64, 3, 2, 1, ['igemm_*_walk*'], stats=True)),
    ('dgrad-conv3x3_c128', {}, lambda: dgrad_case('conv3x3_c128 dgrad', 3, 24, 40, 128, 128, 3, 1, 1, ['conv3x3_c128'])),
    ('dgrad-dgrad3x3s2_k64c32', {}, lambda: dgrad_case('dgrad3x3s2_k64c32', 2, 32, 64, 32, 64, 3, 2, 1, ['dgrad3x3s2_k64c32'])),
    ('dgrad-dgrad3x3s2_k128c64', {}, lambda: dgrad_case('dgrad3x3s2_k128c64', 2, 32, 64, 64, 128, 3, 2, 1, ['dgrad3x3s2_k128c64'])),
    ('dgrad-deep', {'HDY_NO_CONV3X3_C128': 1, **D0}, lambda: dgrad_case('deep dgrad', 3, 40, 40, 128, 256, 3, 1, 1, ['deep_256x*'])),
    ('dgrad-deep_walk', {'HDY_DEEP_WALK': 1, **D0}, lambda: dgrad_case('deep stride-2 walk', 2, 48, 48, 128, 256, 3, 2, 1, ['deep_256x*_walk'])),
    # weight gradient (accumulate = 0); more than 48 splits reach the unrolled loop of wgrad_reduce_kernel
    ('wgrad-generic-19splits', {}, lambda: wgrad_case('wgrad_generic (19 splits)', 3, 40, 40, 256, 512, 1, 1, 0, ['wgrad_generic', 'wgrad_reduce'], splits=19)),
    ('wgrad-generic-72splits', {}, lambda: wgrad_case('wgrad_generic (72 splits)', 2, 96, 96, 64, 64, 1, 1, 0, ['wgrad_generic', 'wgrad_reduce'], splits=72)),
    ('wgrad-generic-scalar_reduce', {}, lambda: wgrad_case('wgrad_generic (scalar reduce)', 2, 20, 20, 64, 32, 1, 1, 0, ['wgrad_generic', 'wgrad_reduce_scalar'],
                                                           unaligned=True)),
    ('wgrad-generic-fp32', {}, lambda: wgrad_case('wgrad_generic fp32', 2, 20, 20, 32, 32, 3, 2, 1, ['wgrad_generic'], dtype=F32)),
    ('wgrad-wgrad3x3', {}, lambda: wgrad_case('wgrad3x3', 2, 16, 32, 64, 64, 3, 1, 1, ['wgrad3x3'])),
    ('wgrad-wgrad_deep', {}, lambda: wgrad_case('wgrad_deep', 4, 96, 96, 64, 256, 3, 2, 1, ['wgrad_deep'])),
    ('wgrad-stem', {}, lambda: wgrad_stem_case('wgrad_stem', 2, 32, 64, 32, False)),
    ('wgrad-stem_fused', {}, lambda: wgrad_stem_case('wgrad_stem_fused', 3, 64, 128, 32, True)),
    # test_gpu_kernels.py::test_conv_fwd_dgrad_wgrad[case10-bf16] (256 -> 512 1x1, 3 x 40 x 40): the three legs separately, written and in the
    # accumulating form conv_case calls (epilogue added to ones, data gradient to ones, weight gradient to 0 / 2)
    ('case10-fwd', {}, lambda: conv_fwd_case('case10 forward', 3, 40, 40, 256, 512, 1, 1, 0, ['igemm_*'])),
    ('case10-fwd-acc', {}, lambda: conv_fwd_case('case10 forward, accumulating epilogue', 3, 40, 40, 256, 512, 1, 1, 0, ['igemm_*'], accumulate=True)),
    ('case10-dgrad', {}, lambda: dgrad_case('case10 data gradient', 3, 40, 40, 256, 512, 1, 1, 0, ['igemm_*'])),
    ('case10-dgrad-acc', {}, lambda: dgrad_case('case10 data gradient, accumulating', 3, 40, 40, 256, 512, 1, 1, 0, ['igemm_*'], accumulate=True)),
    ('case10-wgrad-acc', {}, lambda: wgrad_case('case10 weight gradient, accumulating', 3, 40, 40, 256, 512, 1, 1, 0, ['wgrad_generic', 'wgrad_reduce'],
                                                splits=19, accumulate=True)),
    # fused 1x1 backward
    ('fused1x1-64-pair', {}, lambda: fused_1x1_case('conv1x1_bwd_64 pair', 64, 2, 4099, True)),
    ('fused1x1-64-stats', {}, lambda: fused_1x1_case('conv1x1_bwd_64 + statistics', 64, 1, 128 * 1100 + 33, False, stats=True)),
    ('fused1x1-96', {}, lambda: fused_1x1_case('conv1x1_bwd_96', 96, 4, 19200, False)),
    ('fused1x1-32', {}, lambda: fused_1x1_case('conv1x1_bwd_32', 32, 1, 128 * 3 + 37, False)),
    # BatchNorm
    ('bn_finalize-1stage', {}, lambda: bn_finalize_case('hdy_bn_finalize (one stage)', 37, 64)),
    ('bn_finalize-2stage', {}, lambda: bn_finalize_case('hdy_bn_finalize (two stages)', 1500, 48)),
    ('bn_finalize_pair-1stage', {}, lambda: bn_finalize_case('hdy_bn_finalize_pair (one stage)', 20, 96, Ka=32)),
    ('bn_finalize_pair-2stage', {}, lambda: bn_finalize_case('hdy_bn_finalize_pair (two stages)', 2049, 64, Ka=40)),
    ('bn_act_bwd-reduce4-few_blocks', {}, lambda: bn_act_bwd_case('hdy_bn_act_bwd bf16 reduce4, 2 blocks', 100, 64, BF16, 2, 'bn_bwd_reduce4')),
    ('bn_act_bwd-reduce4-1024_blocks', {}, lambda: bn_act_bwd_case('hdy_bn_act_bwd bf16 reduce4, 1024 blocks', 1024 * 256 + 77, 32, BF16, 1024, 'bn_bwd_reduce4')),
    ('bn_act_bwd-generic_bf16-few_blocks', {'HDY_NO_BN_REDUCE4': 1},
     lambda: bn_act_bwd_case('hdy_bn_act_bwd bf16 generic, 2 blocks', 100, 64, BF16, 2, 'bn_bwd_reduce')),
    ('bn_act_bwd-generic_bf16-1024_blocks', {'HDY_NO_BN_REDUCE4': 1},
     lambda: bn_act_bwd_case('hdy_bn_act_bwd bf16 generic, 1024 blocks', 1024 * 256 + 77, 32, BF16, 1024, 'bn_bwd_reduce')),
    ('bn_act_bwd-fp32-few_blocks', {}, lambda: bn_act_bwd_case('hdy_bn_act_bwd fp32, 2 blocks', 100, 48, F32, 2, 'bn_bwd_reduce')),
    ('bn_act_bwd-fp32-1024_blocks', {}, lambda: bn_act_bwd_case('hdy_bn_act_bwd fp32, 1024 blocks', 1024 * 256 + 77, 32, F32, 1024, 'bn_bwd_reduce')),
    ('bn_bwd_finalize_slabs-small', {}, lambda: bn_bwd_finalize_slabs_case('hdy_bn_bwd_finalize_slabs', 37, 64)),
    ('bn_bwd_finalize_slabs-large', {}, lambda: bn_bwd_finalize_slabs_case('hdy_bn_bwd_finalize_slabs (>= 1024 slabs)', 1500, 48)),
    ('colsum-bf16-small', {}, lambda: colsum_case('hdy_colsum bf16', 90, 64, BF16, 2)),
    ('colsum-fp32-large', {}, lambda: colsum_case('hdy_colsum fp32 (1024 blocks)', 1024 * 256 + 5, 40, F32, 1024)),
    # segmentation branch: GroupNorm and soft-dice workspaces
    ('seg-groupnorm_fwd-bf16', {}, lambda: groupnorm_case('hdy_groupnorm_fwd bf16', 2, 12, 10, 64, 32, BF16, False)),
    ('seg-groupnorm_fwd-fp32', {}, lambda: groupnorm_case('hdy_groupnorm_fwd fp32', 1, 40, 24, 128, 32, F32, False)),
    ('seg-groupnorm_bwd-bf16', {}, lambda: groupnorm_case('hdy_groupnorm_bwd bf16', 2, 12, 10, 64, 32, BF16, True)),
    ('seg-groupnorm_bwd-fp32', {}, lambda: groupnorm_case('hdy_groupnorm_bwd fp32', 2, 9, 9, 24, 4, F32, True)),
    ('seg-softdice', {}, lambda: softdice_case('hdy_softdice', 3, 173, 211, 3)),
    # SPPF pools and the upsample (pool.hip): LDS planes with borders the kernels fill themselves, outputs written whole
    ('sppf-keys32-bwd_c16', {}, lambda: sppf_case('SPPF bf16, 32-channel keys', 2, 20, 20, 64, BF16, ['sppf_fwd_keys32_pos', 'sppf_bwd_c16'])),
    ('sppf-keys16-bwd_c8_two', {}, lambda: sppf_case('SPPF bf16, 16-channel keys', 1, 32, 32, 48, BF16, ['sppf_fwd_keys16_pos', 'sppf_bwd_c8_two'])),
    ('sppf-float32', {'HDY_SPPF_NO_KEYS': 1}, lambda: sppf_case('SPPF bf16, 32-channel float compare', 2, 20, 20, 32, BF16, ['sppf_fwd_float32_pos', 'sppf_bwd_c16'])),
    ('sppf-float16', {'HDY_SPPF_NO_KEYS': 1}, lambda: sppf_case('SPPF bf16, 16-channel float compare', 1, 27, 27, 16, BF16, ['sppf_fwd_float16_pos', 'sppf_bwd_c8_two'])),
    ('sppf-c8-fp32', {}, lambda: sppf_case('SPPF fp32, 8 channels, one position plane', 1, 40, 40, 24, F32, ['sppf_fwd_c8_pos', 'sppf_bwd_c8_one'])),
    ('upsample-bf16', {}, lambda: upsample_case('upsample bf16', 2, 5, 6, 24, BF16)),
    ('upsample-fp32', {}, lambda: upsample_case('upsample fp32', 3, 7, 5, 12, F32)),
]
ROW_IDS = [r[0] for r in ROWS]


def _build(row):
    """the row's case, built under its kernel-selection options; the returned ExitStack keeps them set for the runs"""
    rid, opts, builder = row
    es = ExitStack()
    try:
        for k, v in opts.items():
            es.enter_context(_lib.option(k, v))
        return builder(), es
    except BaseException:
        es.close()
        raise


@pytest.mark.timeout(120)
@pytest.mark.parametrize('row', ROWS, ids=ROW_IDS)
def test_poisoned_scratch_does_not_reach_outputs(row):
    case, es = _build(row)
    with es:
        res = {}
        for pat in 'ABC':
            res[pat] = run_case(case, pat)
            check_untouched(case, pat)
        for pat in 'BC':
            for label, a in res['A'][0].items():
                b = res[pat][0][label]
                n = (a != b).sum().item()
                assert n == 0, f'{case.name}: {n} elements of output {label} differ between scratch pattern A and {pat} (a read of memory the call did not write)'
        assert_families(case, res['A'][1])
        assert res['A'][1] == res['B'][1] == res['C'][1]
        case.check()


_OTHER = {}


def _other_family():
    """a launch of another kernel family (an igemm forward with statistics and a BatchNorm backward) on its own buffers"""
    if 'recs' not in _OTHER:
        N, H, W, C, K = 4, 48, 48, 96, 96
        x = to_dev_nhwc(q(rnd((N, C, H, W), 91), BF16), BF16)
        wp = ops.pack_alloc(K, C, 3, 3, 1, 1, ops.PACK_FWD, BF16, DEV)
        ops.run([ops.rec_pack(rnd((K, C, 3, 3), 92, 0.05).to(DEV), None, 1, 1, ops.PACK_FWD, wp)])
        y = torch.empty((N, H, W, K), dtype=BF16, device=DEV)
        st = torch.empty((ops.stat_slabs(N, H, W, C, K, 3, 3, 1, 1, BF16), 2, K), device=DEV)
        M = N * H * W
        v = torch.ones(K, device=DEV)
        ws = torch.empty(ops.bn_bwd_ws_floats(M, K), device=DEV)
        dy = torch.empty_like(y)
        _OTHER['recs'] = [ops.rec_conv_fwd(x, wp, y, K, 3, 3, 1, 1, stats=st),
                          ops.rec_bn_act_bwd(x, y, v, v * 0, v * 0, v, dy, torch.empty(K, device=DEV), torch.empty(K, device=DEV), ws)]
        _OTHER['side'] = torch.cuda.Stream(device=DEV)
    return _OTHER['recs'], _OTHER['side']


@pytest.mark.timeout(120)
@pytest.mark.parametrize('row', ROWS, ids=ROW_IDS)
def test_repeats_are_bit_identical(row):
    case, es = _build(row)
    with es:
        recs, side = _other_family()
        first, _ = run_case(case, 'B')
        for r in range(1, REPEATS):
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream())
            side.wait_event(ev)
            ops.run(recs[:1 + r % 2], stream=side.cuda_stream)         # runs beside the row's launches
            got, _ = run_case(case, 'B')
            torch.cuda.current_stream().wait_stream(side)
            for label, a in first.items():
                n = (a != got[label]).sum().item()
                assert n == 0, f'{case.name}: repeat {r}: {n} elements of output {label} differ from the first run'
        torch.cuda.synchronize()


# ---------------------------------------------------------------------------------- direct references for entry points reached only through the model
@pytest.mark.timeout(60)
def test_syncbn_sums_chain_equals_the_local_finalize_and_backward_coefficients():
    """hdy_bn_slab_sums -> hdy_bn_finalize_sums (a pair split at Ka) equals hdy_bn_finalize_pair on the same slabs, and hdy_bn_slab_sums over the
    BatchNorm-backward partial slabs -> hdy_bn_bwd_coeffs_sums equals the c1 / c2 of hdy_bn_act_bwd (one rank: the all-reduce is the identity)"""
    mt, K, Ka, count = 37, 96, 40, 37 * 100
    g = torch.Generator().manual_seed(4)
    stats = torch.stack([torch.randn((mt, K), generator=g) * 10, torch.rand((mt, K), generator=g) * 100 + 60], 1).to(DEV)
    outs = []
    for sync in (False, True):
        gamma, beta, rm, rv = (t.to(DEV) for t in _bn_params(K, 3))
        o = [torch.full((K,), float('nan'), device=DEV) for _ in range(4)]
        bn_a, bn_b = (gamma[:Ka], beta[:Ka], rm[:Ka], rv[:Ka]), (gamma[Ka:], beta[Ka:], rm[Ka:], rv[Ka:])
        if sync:
            sums = torch.full((2 * K + 1,), float('nan'), dtype=torch.float64, device=DEV)
            ops.run([ops.rec_bn_slab_sums(stats, mt, K, count, sums), ops.rec_bn_finalize_sums(sums, K, 0, K, Ka, bn_a, bn_b, *o)])
            s = stats.double().sum(0).cpu()
            assert_close(sums[:2 * K].cpu().view(2, K), s, 1e-6, 'slab sums')
            assert sums[2 * K].item() == count
        else:
            ops.run([ops.rec_bn_finalize_pair(stats, mt, K, Ka, count, bn_a, bn_b, *o)])
        torch.cuda.synchronize()
        outs.append([t.cpu() for t in o + [rm, rv]])
    for a, b, what in zip(*outs, ('scale', 'shift', 'mean', 'invstd', 'running_mean', 'running_var')):
        assert_close(b, a, 1e-6, f'finalize_sums vs finalize_pair: {what}')
    # backward coefficients
    M = 5000
    dz, y, scale, shift, mean, invstd = _bn_bwd_operands(M, 64, BF16, seed=11)
    d = lambda t: t.to(DEV)
    ws = torch.full((ops.bn_bwd_ws_floats(M, 64),), float('nan'), device=DEV)
    dg, db = torch.zeros(64, device=DEV), torch.zeros(64, device=DEV)
    ops.run([ops.rec_bn_act_bwd(to_dev_nhwc(dz, BF16), to_dev_nhwc(y, BF16), d(scale), d(shift), d(mean), d(invstd), None, dg, db, ws)])
    nb = ops.bn_bwd_blocks(M)
    sums = torch.full((2 * 64 + 1,), float('nan'), dtype=torch.float64, device=DEV)
    c1, c2 = torch.full((64,), float('nan'), device=DEV), torch.full((64,), float('nan'), device=DEV)
    ops.run([ops.rec_bn_slab_sums(ws[:nb * 2 * 64].view(nb, 2, 64), nb, 64, M, sums), ops.rec_bn_bwd_coeffs_sums(sums, 64, c1, c2)])
    r1, r2 = ops.bn_bwd_coeffs(ws, M, 64)
    torch.cuda.synchronize()
    assert_close(c1.cpu(), r1.cpu(), 1e-6, 'c1 from the sums')
    assert_close(c2.cpu(), r2.cpu(), 1e-6, 'c2 from the sums')
    du, xh = _bn_bwd_ref(dz, y, scale, shift, mean, invstd)
    assert_close(c1.cpu(), du.mean(0).float(), 2e-3, 'c1 vs fp64')
    assert_close(c2.cpu(), (du * xh).mean(0).float(), 2e-3, 'c2 vs fp64')


@pytest.mark.timeout(60)
@pytest.mark.parametrize('dtype', [F32, BF16])
@pytest.mark.parametrize('two', [False, True])
def test_bn_act_bwd_apply_against_fp64(two, dtype):
    """hdy_bn_act_bwd_apply: dy = scale * (du - c1 - xhat * c2), du = dz * SiLU'(scale * y + shift), dz from one or two sources split at Ka"""
    M, K, Ka = 3000, 64, 24
    dz, y, scale, shift, mean, invstd = _bn_bwd_operands(M, K, dtype, seed=21)
    c1, c2 = rnd((K,), 28, 0.2), rnd((K,), 29, 0.2)
    d = lambda t: t.to(DEV)
    if two:
        dza, dzb = to_dev_nhwc(dz[:, :Ka], dtype, ld=Ka + 8, off=8), to_dev_nhwc(dz[:, Ka:], dtype, ld=K, off=0)
    else:
        dza, dzb = to_dev_nhwc(dz, dtype, ld=K + 8, off=0), None
    dy = to_dev_nhwc(torch.zeros((1, K, 1, M)), dtype, ld=K + 16, off=8)
    ops.run([ops.rec_bn_act_bwd_apply(dza, dzb, to_dev_nhwc(y, dtype), d(scale), d(shift), d(mean), d(invstd), d(c1), d(c2), dy)])
    du, xh = _bn_bwd_ref(dz, y, scale, shift, mean, invstd)
    ref = scale.double() * (du - c1.double() - xh * c2.double())
    assert_close(dy.float().cpu().reshape(M, K), ref.float(), TOL[dtype], 'bn_act_bwd_apply')
    assert dy._base[..., :8].float().eq(7.0).all() and dy._base[..., 8 + K:].float().eq(7.0).all()


@pytest.mark.timeout(60)
@pytest.mark.parametrize('dtype', [F32, BF16])
@pytest.mark.parametrize('M', [90, 1024 * 256 + 5])
@pytest.mark.parametrize('acc', [False, True])
def test_colsum_against_fp64(M, acc, dtype):
    K = 40 if dtype == F32 else 48
    dz = q(rnd((1, K, 1, M), 3), dtype)
    ws = torch.full((ops.bn_bwd_ws_floats(M, K),), float('nan'), device=DEV)
    base = rnd((K,), 4)
    out = base.to(DEV) if acc else torch.full((K,), float('nan'), device=DEV)
    ops.run([ops.rec_colsum(to_dev_nhwc(dz, dtype, ld=K + 8, off=8), out, ws, accumulate=acc)])
    ref = dz.double().sum((0, 2, 3)) + (base.double() if acc else 0)
    assert_close(out.cpu(), ref.float(), 1e-5, 'colsum')


@pytest.mark.timeout(60)
@pytest.mark.parametrize('dtype', [F32, BF16])
def test_det_grad_pack_equals_the_reshape(dtype):
    """hdy_det_grad_pack: the logits gradient (B, na, ny, nx, no), any strides -> NHWC (B, ny, nx, ld) with channel a * no + o; the padding
    channels [na * no, ld) are written as zeros"""
    B, na, ny, nx, no, ld = 2, 3, 7, 9, 13, 48
    g = rnd((B, ny, nx, na, no), 5).to(DEV).permute(0, 3, 1, 2, 4)          # the strides of the plan's pixel-major logits view
    out = torch.full((B, ny, nx, ld), float('nan'), dtype=dtype, device=DEV)
    ops.run([ops.rec_det_grad_pack(g, out, na, no)])
    want = g.permute(0, 2, 3, 1, 4).reshape(B, ny, nx, na * no).to(dtype)
    assert torch.equal(out[..., :na * no], want)
    assert (out[..., na * no:].float() == 0).all() and not torch.signbit(out[..., na * no:].float()).any()
    gc = g.contiguous()                                                        # a contiguous gradient: other strides, same result
    out2 = torch.full_like(out, float('nan'))
    ops.run([ops.rec_det_grad_pack(gc, out2, na, no)])
    assert torch.equal(out2, out)


@pytest.mark.timeout(60)
@pytest.mark.parametrize('dtype', [F32, BF16])
def test_scale_inplace_relu_bwd_and_bilinear_bwd_h(dtype):
    """hdy_scale_inplace (t *= s), hdy_relu_bwd (du = dz where y > 0) and the H pass of the resize backward (ops.bilinear_bwd_h) against torch"""
    n = 4099 * 8
    t0 = rnd((n,), 1, 3.0).to(dtype)
    t = t0.to(DEV)
    s = torch.tensor([0.37], device=DEV)
    ops.scale_inplace(t, s)
    torch.cuda.synchronize()
    assert t.dtype == dtype
    want = (t0.float() * s.cpu()).to(dtype)                                       # one fp32 product, one rounding
    assert torch.equal(t.cpu().view(INT_VIEW[dtype]), want.view(INT_VIEW[dtype])), 'scale_inplace'
    dz, y = rnd((n,), 2).to(dtype), rnd((n,), 3).to(dtype)
    y[::7] = 0.0                                                                  # ties at zero: no gradient
    du = ops.relu_bwd(dz.to(DEV), y.to(DEV))
    assert du.dtype == dtype
    assert torch.equal(du.cpu(), torch.where(y > 0, dz, torch.zeros_like(dz)))
    N, Hi, Ho, Wi, C = 2, 9, 40, 6, 16
    dw = q(rnd((N, C, Ho, Wi), 4), dtype)
    xr = torch.zeros((N, C, Hi, Wi), requires_grad=True)
    F.interpolate(xr, size=(Ho, Wi), mode='bilinear', align_corners=True).backward(dw)
    for acc in (False, True):
        out = to_dev_nhwc(torch.ones((N, C, Hi, Wi)), dtype, ld=C + 8, off=8)
        if not acc:
            out.fill_(float('nan'))
        ops.bilinear_bwd_h(to_dev_nhwc(dw, dtype), Hi, out, accumulate=acc)
        assert_close(from_dev_nhwc(out), xr.grad + (1.0 if acc else 0.0), TOL[dtype] * 2, f'bilinear_bwd_h accumulate={acc}')
        assert out._base[..., :8].float().eq(7.0).all()
