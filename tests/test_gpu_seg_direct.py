"""csrc/seg.hip driven directly (the C entry points through _lib.call, our own buffers and pitches, no model) on an MI355X against the float64
restatement tests/segk_ref.py, on the cases of tests/segk_cases.py (tests/test_segk_ref_host.py proves on the CPU what each contains).

Every activation lives at a nonzero channel offset of a wider buffer with 7.0 outside, every flat tensor between two 7.0 guards; every output
is prefilled with 7.0, inside too, and so is the workspace.  After each call the 7.0 outside must be intact; inside, the comparison with the
reference shows that the prefill is gone.  NaN and infinities must sit exactly where the restatement has them.

Criteria (derivations in segk_ref): every element within a bound computed from the reference and the launch geometry (no bound comes from a
kernel's output, no element is excluded); kernel form against kernel form: equal bits.

Measured on an MI355X, worst case of each group, error in units of its bound (must stay <= 1):

    group                                      worst error / bound
    groupnorm y / dx / dgamma, dbeta, fp32     0.524 (chunk2-f32) / 0.469 (zeros) / 0.459 (chunk2-f32)     median 0.275 / 0.164 / 0.171 of 11
    groupnorm 'offset', that group alone       y 0.082, dx 0.004: what it uses of a bound that allows rstd 20 % (9 % without the mean^2 term)
    groupnorm y / dx / dgamma, dbeta, bf16     0.995 (chunk2-bf16) / 0.995 (chunk2-bf16) / 0.230 (hw-1)    median 0.969 / 0.979 / 0.087 of 9
    groupnorm nonfinite, fp32                  0.343 / 0.231 / 0.174 (nan)                                 5 cases, patterns equal
    groupnorm nonfinite, bf16                  0.990 / 0.993 (nan-gamma) / 0.119 (nan-dout)                5 cases, patterns equal
    resize forward fp32 / bf16                 0.564 (down-3) / 0.996 (x8-3)                               median 0.363 / 0.996 of 26
    resize transpose fp32 / bf16               0.597 (down-3) / 0.996 (rows-4100-3)                        median 0.220 / 0.981 of 28
    dice loss                                  0.066 (nc8)                                                 median 0.016 of 25
    dice gradient                              0.995 (spread80: flushed probabilities against the floor)   median 0.303 of 24; nan: 0.307
    dice gradient + W pass (softdice_wgrad)    0.122 (rows-4098)                                           median 0.037 of 3
    softmax2d                                  0.321 (nc 3)                                                median 0.307 of 3

115 tests here and the three convolution-epilogue tests of test_gpu_kernels.py: 9.6 s in all, the slowest (resize long-row, bf16, three vectors) 2.2 s.

A bf16 output sits just below 1 by construction: half a bf16 ulp is nearly all of its bound and some element always rounds that far.
Left out: the grid cap of dice_bwd_kernel, which needs more than 4.19 M pixels in one image.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import segk_cases as sc  # noqa: E402
import segk_ref as ref  # noqa: E402
from hd_yolo_amd import _lib, ops  # noqa: E402

DEV = torch.device('cuda', 0)
GUARD = 8                                     # floats (or elements) of 7.0 before and after a flat tensor; channels around an activation
INT_VIEW = {torch.float32: torch.int32, torch.bfloat16: torch.int16}


def bits(t):
    return t.contiguous().view(INT_VIEW[t.dtype])


def figure(group, what, worst):
    print(f'SEGFIG {group} | {what} | {worst:.3f}')
    return worst


class Act:
    """an activation [..., C] at channel `off` of a pitch C + off + tail buffer, 7.0 everywhere else (a=None: 7.0 inside too, an output's prefill)"""

    def __init__(self, a, dt, shape=None, off=GUARD, tail=GUARD):
        shape = tuple(a.shape) if a is not None else tuple(shape)
        self.C, self.off, self.shape = shape[-1], off, shape
        self.buf = torch.full(shape[:-1] + (shape[-1] + off + tail,), sc.POISON, dtype=sc.TORCH[dt], device=DEV)
        self.v = self.buf[..., off:off + self.C]
        if a is not None:
            self.v.copy_(torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(sc.TORCH[dt]))
        self.ptr, self.ld = self.v.data_ptr(), self.buf.shape[-1]

    def host(self):
        return self.v.float().cpu().numpy().astype(np.float64)

    def intact(self):
        assert (self.buf[..., :self.off] == sc.POISON).all() and (self.buf[..., self.off + self.C:] == sc.POISON).all(), 'poison outside the view overwritten'


class Flat:
    """a contiguous fp32 tensor between two guards of 7.0 (a=None: prefilled output)"""

    def __init__(self, a=None, shape=None):
        shape = tuple(np.shape(a)) if a is not None else tuple(shape)
        n = int(np.prod(shape))
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), sc.POISON, dtype=torch.float32, device=DEV)
        self.v = self.buf[GUARD:GUARD + n].view(shape)
        if a is not None:
            self.v.copy_(torch.from_numpy(np.ascontiguousarray(a, np.float32)))
        self.ptr = self.v.data_ptr()

    def host(self):
        return self.v.cpu().numpy().astype(np.float64)

    def intact(self):
        assert (self.buf[:GUARD] == sc.POISON).all() and (self.buf[GUARD + self.n:] == sc.POISON).all(), 'poison around a tensor overwritten'


def call(name, *args):
    """-> the kernel families the library noted"""
    _lib.dispatch_log(reset=True)
    _lib.call(name, *args, ops.stream_ptr())
    torch.cuda.synchronize()
    return _lib.dispatch_log(reset=True)


def dcode(dt):
    return ops.dcode(sc.TORCH[dt])


# ------------------------------------------------------------------------------------------ GroupNorm
@pytest.mark.parametrize('case', sc.GN_CASES, ids=sc.case_id)
def test_groupnorm_matches_the_float64_restatement(case):
    """forward and backward with relu 0 and 1, the parameter gradients stored and accumulated; the backward runs from the forward kernel's own
    stat / ab.  With relu = 1 a NaN or an infinity in x must come out as a NaN (image, group), not as zeros."""
    name, dt = case
    c, g = sc.gn_inputs(name, dt), sc.GN[name]
    N, HW, C, G = g['N'], g['HW'], g['C'], g['G']
    n, bf = sc.gn_geometry(N, HW, C, sc.VE[dt])['n'], dt == 'bf16'
    x, dout, gamma, beta = Act(c['x'], dt), Act(c['dout'], dt, off=16, tail=0), Flat(c['gamma']), Flat(c['beta'])
    wsf = _lib.query('hdy_groupnorm_workspace_floats', N, C)
    assert wsf == N * sc.GN_SLICES * 2 * C + N * 2 * C
    ws = torch.empty(wsf + GUARD, device=DEV)
    bfw = ref.gn_forward_bound(c['x'], c['gamma'], c['beta'], G, sc.GN_EPS, n)
    worst = {'y': 0.0, 'dx': 0.0, 'param': 0.0}
    far = slice(C // G, 2 * C // G)                                             # 'offset': the channels of the group with |mean| = 1000 std
    worst_far = {'y': 0.0, 'dx': 0.0}
    for relu in (0, 1):
        y, stat, ab = Act(None, dt, (N, HW, C), off=24), Flat(shape=(N, G, 2)), Flat(shape=(N, 2, C))
        ws.fill_(sc.POISON)
        log = call('hdy_groupnorm_fwd', x.ptr, x.ld, gamma.ptr, beta.ptr, y.ptr, y.ld, stat.ptr, ab.ptr, N, HW, C, G, sc.GN_EPS, relu, dcode(dt),
                   ws.data_ptr(), wsf)
        assert log == ['groupnorm_fwd'], log
        ry, _ = ref.gn_forward(c['x'], c['gamma'], c['beta'], G, sc.GN_EPS, relu)
        worst['y'] = max(worst['y'], ref.check(y.host(), ry, ref.finish(bfw, ry, bf), f'{case} relu {relu} y'))
        if name == 'offset':
            worst_far['y'] = max(worst_far['y'], ref.ratios(y.host(), ry, ref.finish(bfw, ry, bf))[:, :, far].max())
        for t in (x, y, gamma, beta, stat, ab):
            t.intact()
        assert (ws[wsf:] == sc.POISON).all()
        rdx, rdg, rdb = ref.gn_backward(c['dout'], c['x'], c['gamma'], c['beta'], G, sc.GN_EPS, relu)
        bdx, bdg, bdb = ref.gn_backward_bounds(c['dout'], c['x'], c['gamma'], c['beta'], G, sc.GN_EPS, relu, n)
        for acc in (0, 1):
            dx, coef = Act(None, dt, (N, HW, C), off=8, tail=24), Flat(shape=(N, 3, C))
            dg, db = (Flat(c[k]) for k in ('old_dg', 'old_db')) if acc else (Flat(shape=(C,)), Flat(shape=(C,)))
            ws.fill_(sc.POISON)
            log = call('hdy_groupnorm_bwd', dout.ptr, dout.ld, x.ptr, x.ld, gamma.ptr, stat.ptr, ab.ptr, dx.ptr, dx.ld, dg.ptr, db.ptr, acc, coef.ptr,
                       N, HW, C, G, relu, dcode(dt), ws.data_ptr(), wsf)
            assert log == ['groupnorm_bwd'], log
            what = f'{case} relu {relu} accumulate {acc}'
            worst['dx'] = max(worst['dx'], ref.check(dx.host(), rdx, ref.finish(bdx, rdx, bf), what + ' dx'))
            if name == 'offset':
                worst_far['dx'] = max(worst_far['dx'], ref.ratios(dx.host(), rdx, ref.finish(bdx, rdx, bf))[:, :, far].max())
            og, ob = (c['old_dg'].astype(np.float64), c['old_db'].astype(np.float64)) if acc else (None, None)
            tg, tb = (rdg + og, rdb + ob) if acc else (rdg, rdb)
            worst['param'] = max(worst['param'], ref.check(dg.host(), tg, ref.gn_param_bound(bdg, tg, og), what + ' dgamma'),
                                 ref.check(db.host(), tb, ref.gn_param_bound(bdb, tb, ob), what + ' dbeta'))
            for t in (x, dout, dx, gamma, stat, ab, coef, dg, db):
                t.intact()
            assert (ws[wsf:] == sc.POISON).all()
    assert np.array_equal(x.host(), c['x'].astype(np.float64), equal_nan=True) and np.array_equal(dout.host(), c['dout'].astype(np.float64), equal_nan=True)
    for k, v in worst.items():
        figure(f'groupnorm {k} {dt}' + (' nonfinite' if name in sc.GN_NONFINITE else ''), name, v)
    if name == 'offset':
        for k, v in worst_far.items():
            figure(f'groupnorm {k} f32, the offset group alone', name, v)


# ------------------------------------------------------------------------------------------ resize
def _axis(src, dst, outer, Ai, Ao, inner, C, acc, dt):
    assert call('hdy_bilinear_bwd_axis', src.ptr, src.ld, dst.ptr, dst.ld, outer, Ai, Ao, inner, C, acc, dcode(dt)) == []


def _dead_inputs_exact(t, dead_h, dead_w, base, dt, what):
    """inputs that no output touches (in the kernel's own fp32 index arithmetic): +0 bits when stored, the bits they held when accumulated"""
    want = torch.from_numpy(np.ascontiguousarray(base, np.float32)).to(sc.TORCH[dt]) if base is not None else torch.zeros(t.shape, dtype=sc.TORCH[dt])
    got = t.v.cpu()
    for sel in ((slice(None), dead_h), (slice(None), slice(None), dead_w)):
        if len(sel[-1]):
            assert torch.equal(bits(got[sel]), bits(want[sel])), f'{what}: an input that receives no gradient is not ' + ('unchanged' if base is not None else '0')


@pytest.mark.parametrize('case', sc.RESIZE_CASES, ids=sc.case_id)
def test_resize_matches_the_float64_restatement(case):
    """forward stored and accumulated; the transpose in the form ops.bilinear_bwd selects (bit-equal to that wrapper), stored and accumulated;
    the W pass and the H pass driven separately through hdy_bilinear_bwd_axis, the W pass's result checked on its own.  Inputs that receive
    no gradient (downsizing) come out as exact zeros, or bit for bit unchanged under accumulate, in every form."""
    name, dt, nv = case
    N, (Hi, Wi), (Ho, Wo) = sc.RESIZE[name]
    c, C, bf = sc.resize_inputs(name, dt, nv), nv * sc.VE[dt], dt == 'bf16'
    x, dy = Act(c['x'], dt), Act(c['dy'], dt, off=16, tail=0)
    ry, by = ref.resize_forward(c['x'], (Ho, Wo))
    form = sc.bwd_form((Hi, Wi), (Ho, Wo))
    rdx = ref.resize_backward(c['dy'], (Hi, Wi))
    bdx = ref.resize_backward_bound(c['dy'], (Hi, Wi), form, bf)
    worst = {'forward': 0.0, 'transpose': 0.0}
    dead_h = [i for i in range(Hi) if not len(sc.contributors32(i, Hi, Ho))]
    dead_w = [i for i in range(Wi) if not len(sc.contributors32(i, Wi, Wo))]
    assert name != 'down' or dead_h == dead_w == [1, 14]
    for acc in (0, 1):
        y = Act(c['base'] if acc else None, dt, (N, Ho, Wo, C), off=24)
        assert call('hdy_bilinear_fwd', x.ptr, x.ld, y.ptr, y.ld, N, Hi, Wi, Ho, Wo, C, acc, dcode(dt)) == []
        total = ry + c['base'] if acc else ry
        worst['forward'] = max(worst['forward'], ref.check(y.host(), total, ref.finish(by, total, bf, c['base'] if acc else None), f'{case} forward accumulate {acc}'))
        dx = Act(c['dbase'] if acc else None, dt, (N, Hi, Wi, C), off=8, tail=24)
        if form == 'two-pass':
            tmp = Act(None, dt, (N, Ho, Wi, C))
            _axis(dy, tmp, N * Ho, Wi, Wo, 1, C, 0, dt)
            _axis(tmp, dx, N, Hi, Ho, Wi, C, acc, dt)
            tmp.intact()
        else:
            assert call('hdy_bilinear_bwd', dy.ptr, dy.ld, dx.ptr, dx.ld, N, Hi, Wi, Ho, Wo, C, acc, dcode(dt)) == []
        total = rdx + c['dbase'] if acc else rdx
        worst['transpose'] = max(worst['transpose'], ref.check(dx.host(), total, ref.finish(bdx, total, bf, c['dbase'] if acc else None),
                                                               f'{case} transpose ({form}) accumulate {acc}'))
        via = Act(c['dbase'] if acc else None, dt, (N, Hi, Wi, C))
        ops.bilinear_bwd(dy.v, (Hi, Wi), out=via.v, accumulate=bool(acc))
        torch.cuda.synchronize()
        assert torch.equal(bits(via.v), bits(dx.v)), 'ops.bilinear_bwd runs another form than segk_cases.bwd_form restates'
        _dead_inputs_exact(dx, dead_h, dead_w, c['dbase'] if acc else None, dt, f'{case} ({form}) accumulate {acc}')
        for t in (x, dy, y, dx, via):
            t.intact()
    # the two passes on their own, whatever form the wrapper picks
    tmp, dx = Act(None, dt, (N, Ho, Wi, C), off=24), Act(None, dt, (N, Hi, Wi, C))
    _axis(dy, tmp, N * Ho, Wi, Wo, 1, C, 0, dt)
    rt, bt = ref.resize_backward_axis(c['dy'], Wi, 2)
    worst['transpose'] = max(worst['transpose'], ref.check(tmp.host(), rt, ref.finish(bt, rt, bf), f'{case} W pass'))
    _axis(tmp, dx, N, Hi, Ho, Wi, C, 0, dt)
    b2 = ref.resize_backward_bound(c['dy'], (Hi, Wi), 'two-pass', bf)
    worst['transpose'] = max(worst['transpose'], ref.check(dx.host(), rdx, ref.finish(b2, rdx, bf), f'{case} W pass then H pass'))
    _dead_inputs_exact(tmp, [], dead_w, None, dt, f'{case} W pass')
    _dead_inputs_exact(dx, dead_h, dead_w, None, dt, f'{case} W pass then H pass')
    tmp.intact(), dx.intact(), dy.intact()
    assert np.array_equal(x.host(), c['x'].astype(np.float64)) and np.array_equal(dy.host(), c['dy'].astype(np.float64))
    for k, v in worst.items():
        figure(f'resize {k} {dt}', f'{name}-{nv}', v)


@pytest.mark.parametrize('dt', sc.DTYPES)
def test_lds_w_pass_and_global_axis_kernel_give_equal_bits(dt):
    """the same gradient rows once as one call over three vectors (a row 32 bytes beyond the LDS stage: the global one-axis kernel) and once as
    three calls over one vector each (the LDS kernel), stored and accumulated"""
    e, ve = sc.LDS_EDGE, sc.VE[dt]
    C = e['nv'] * ve
    rng = np.random.RandomState(3)
    g = sc.rounded(rng.uniform(-1, 1, (1, e['rows'], e['Ao'], C)), dt)
    old = sc.rounded(rng.uniform(-1, 1, (1, e['rows'], e['Ai'], C)), dt)
    dy = Act(g, dt)
    rt, bt = ref.resize_backward_axis(g, e['Ai'], 2)
    for acc in (0, 1):
        a, b = (Act(old if acc else None, dt, old.shape, off=16) for _ in range(2))
        _axis(dy, a, e['rows'], e['Ai'], e['Ao'], 1, C, acc, dt)
        for k in range(e['nv']):
            esz = a.v.element_size()
            assert call('hdy_bilinear_bwd_axis', dy.ptr + k * ve * esz, dy.ld, b.ptr + k * ve * esz, b.ld, e['rows'], e['Ai'], e['Ao'], 1, ve, acc, dcode(dt)) == []
        assert torch.equal(bits(a.v), bits(b.v))
        total = rt + old if acc else rt
        figure(f'resize transpose {dt}', f'lds-edge accumulate {acc}', ref.check(a.host(), total, ref.finish(bt, total, dt == 'bf16', old if acc else None), 'W pass'))
        a.intact(), b.intact(), dy.intact()


# ------------------------------------------------------------------------------------------ soft dice
def _softdice(c, logits, targets, cw, up, dl, ws, wsf):
    loss = Flat(shape=(1,))
    log = call('hdy_softdice', logits.ptr, c['ld'], targets.ptr, cw.ptr if cw else None, c['N'], c['HW'], c['nc'], loss.ptr, up.ptr if up else None,
               dl.ptr if dl else None, c['ld'], ws.data_ptr(), wsf)
    assert log == ['softdice'], log
    loss.intact()
    assert (ws[wsf:] == sc.POISON).all()
    return loss


@pytest.mark.parametrize('name', list(sc.DICE))
def test_softdice_matches_the_float64_restatement(name):
    """loss and gradient; the padding channels of the gradient: exact zeros where whole 4-float pixels are stored, untouched elsewhere.  'nan': the
    loss and the gradient of the image that holds it are NaN, the other images' gradients finite and within bound."""
    c = sc.dice_inputs(name)
    N, HW, nc, ld = c['N'], c['HW'], c['nc'], c['ld']
    geo = sc.dice_geometry(HW, nc, ld)
    logits, targets = Flat(c['logits']), Flat(c['targets'])
    cw = Flat(c['cw']) if c['cw'] is not None else None
    up = Flat(np.array([c['upstream']], np.float32)) if c['upstream'] is not None else None
    upv = float(np.float32(c['upstream'])) if c['upstream'] is not None else 1.0
    wsf = _lib.query('hdy_softdice_workspace_floats', N, nc)
    assert wsf == N * sc.DICE_SLICES * 2 * nc + N * 2 * nc
    ws = torch.full((wsf + GUARD,), sc.POISON, device=DEV)
    dl = Flat(shape=(N, HW, ld))
    loss = _softdice(c, logits, targets, cw, up, dl, ws, wsf)
    l = c['logits'][..., :nc]
    rl, rg = ref.dice_loss(l, c['targets'], c['cw']), ref.dice_grad(l, c['targets'], c['cw'], upv)
    bl, bg = ref.dice_bounds(l, c['targets'], c['cw'], upv, geo['n'])
    got = dl.host()
    figure('dice loss', name, ref.check(loss.host(), np.array([rl]), np.array([bl]), f'{name} loss'))
    figure('dice gradient' + (' nan' if c['kind'] == 'nan' else ''), name, ref.check(got[..., :nc], rg, bg, f'{name} gradient'))
    if geo['vector']:
        assert (got[..., nc:4] == 0).all() and (got[..., 4:] == sc.POISON).all(), 'padding of a whole-pixel store'
    else:
        assert (got[..., nc:] == sc.POISON).all(), 'padding gradient touched'
    ws.fill_(sc.POISON)
    only = _softdice(c, logits, targets, cw, up, None, ws, wsf)                 # loss alone (dlogits NULL): the same bits
    assert torch.equal(bits(only.v), bits(loss.v))
    for t in [logits, targets, dl] + [t for t in (cw, up) if t]:
        t.intact()
    assert np.array_equal(logits.host(), c['logits'].astype(np.float64), equal_nan=True)


@pytest.mark.parametrize('name', list(sc.WGRAD))
def test_softdice_wgrad_matches_the_restatement_and_the_two_launches(name):
    """hdy_softdice_wgrad against the restated gradient followed by the restated W pass, and bit for bit against hdy_softdice + the W pass"""
    N, H, W, nc, Wi = sc.WGRAD[name]
    c = sc.dice_inputs(name)
    logits, targets = Flat(c['logits']), Flat(c['targets'])
    cw = Flat(c['cw']) if c['cw'] is not None else None
    wsf = _lib.query('hdy_softdice_workspace_floats', N, nc)
    ws = torch.full((wsf + GUARD,), sc.POISON, device=DEV)
    dl = Flat(shape=(N, H * W, 4))
    loss = _softdice(c, logits, targets, cw, None, dl, ws, wsf)
    want = Flat(shape=(N, H, Wi, 4))
    assert call('hdy_bilinear_bwd_axis', dl.ptr, 4, want.ptr, 4, N * H, Wi, W, 1, 4, 0, dcode('f32')) == []
    ws.fill_(sc.POISON)
    loss2, dw = Flat(shape=(1,)), Flat(shape=(N, H, Wi, 4))
    call('hdy_softdice_wgrad', logits.ptr, targets.ptr, cw.ptr if cw else None, N, H, W, nc, Wi, loss2.ptr, dw.ptr, ws.data_ptr(), wsf)
    assert torch.equal(bits(loss2.v), bits(loss.v)) and torch.equal(bits(dw.v), bits(want.v))
    l = c['logits'][..., :nc]
    g4, b4 = np.zeros((N, H * W, 4)), np.zeros((N, H * W, 4))
    g4[..., :nc] = ref.dice_grad(l, c['targets'], c['cw'], 1.0)
    bl, b4[..., :nc] = ref.dice_bounds(l, c['targets'], c['cw'], 1.0, sc.dice_geometry(H * W, nc, 4)['n'])
    rw, bw = ref.resize_backward_axis(g4.reshape(N, H, W, 4), Wi, 2, b4.reshape(N, H, W, 4))
    figure('dice wgrad', name, max(ref.check(dw.host(), rw, ref.finish(bw, rw, False), f'{name} dw'),
                                   ref.check(loss2.host(), np.array([ref.dice_loss(l, c['targets'], c['cw'])]), np.array([bl]), f'{name} loss')))
    for t in [logits, targets, dl, want, loss2, dw] + ([cw] if cw else []):
        t.intact()
    assert (ws[wsf:] == sc.POISON).all()


@pytest.mark.parametrize('nc,ld', sc.SOFTMAX2D)
def test_softmax2d_matches_the_float64_restatement(nc, ld):
    M, ldp = 1000, nc + 3
    rng = np.random.RandomState(nc)
    l = rng.uniform(-12, 12, (M, ld)).astype(np.float32)
    l[:, nc:] = 80.0                                                            # padding that would win the max
    logits, probs = Flat(l), Flat(shape=(M, ldp))
    assert call('hdy_softmax2d', logits.ptr, ld, probs.ptr, ldp, M, nc) == []
    got = probs.host()
    figure('softmax2d', f'nc {nc}', ref.check(got[:, :nc], ref.softmax(l[:, :nc]), ref.SLACK * ref.softmax_error(l[:, :nc]), f'softmax2d {nc}'))
    assert (got[:, nc:] == sc.POISON).all()
    logits.intact(), probs.intact()
