"""CPU only.  Pins tests/segk_ref.py (the float64 restatement the direct tests of csrc/seg.hip compare with) to torch float64 (F.group_norm,
F.relu, F.interpolate(align_corners=True), torch.softmax + oracle.seg_ref.soft_dice_criterion, autograd for every gradient) at 1e-12 of
the tensor's largest value, pins its NaN / infinity patterns to torch's, proves that every case of tests/segk_cases.py holds the feature it
is named for, and that each comparer accepts half its bound and rejects twice its bound."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import segk_cases as sc
import segk_ref as ref
from oracle import seg_ref

PIN = 1e-12


def pin(got, want, what, scale=0.0):
    got, want = np.asarray(got, np.float64), want.detach().numpy() if torch.is_tensor(want) else np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want)), f'{what}: nonfinite pattern differs from torch'
    fin = np.isfinite(want)
    if fin.any():
        err = np.abs(got[fin] - want[fin]).max()
        assert err <= PIN * max(np.abs(want[fin]).max(), scale, 1e-300), f'{what}: {err:.3g} against a largest value of {np.abs(want[fin]).max():.3g}'


# ------------------------------------------------------------------------------------------ GroupNorm
def torch_gn(c, G, relu):
    x = torch.from_numpy(c['x']).double().permute(0, 2, 1)[..., None].clone().requires_grad_(True)          # [N, C, HW, 1]
    g, b = (torch.from_numpy(c[k]).double().requires_grad_(True) for k in ('gamma', 'beta'))
    y = F.group_norm(x, G, g, b, sc.GN_EPS)
    y = F.relu(y) if relu else y
    y.backward(torch.from_numpy(c['dout']).double().permute(0, 2, 1)[..., None])
    back = lambda t: t.detach()[..., 0].permute(0, 2, 1)                  # noqa: E731
    return back(y), back(x.grad), g.grad, b.grad


@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('case', sc.GN_CASES, ids=sc.case_id)
def test_groupnorm_restatement_equals_torch_float64(case, relu):
    """finite cases at 1e-12; the nonfinite ones by their NaN / infinity pattern as well (pin() compares it always)"""
    name, dt = case
    c, G = sc.gn_inputs(name, dt), sc.GN[name]['G']
    y, dx, dg, db = torch_gn(c, G, relu)
    pin(ref.gn_forward(c['x'], c['gamma'], c['beta'], G, sc.GN_EPS, relu)[0], y, f'{case} y')
    got = ref.gn_backward(c['dout'], c['x'], c['gamma'], c['beta'], G, sc.GN_EPS, relu)
    t = ref.gn_terms(c['dout'], c['x'], c['gamma'], c['beta'], G, sc.GN_EPS, relu)
    k0dy = np.abs(t['k0'] * t['dy'])
    for a, b, what in zip(got, (dx, dg, db), ('dx', 'dgamma', 'dbeta')):                    # dx against its largest term: at HW == 1 it cancels to 0
        pin(a, b, f'{case} relu {relu} {what}', scale=k0dy[np.isfinite(k0dy)].max() if what == 'dx' else 0.0)
    if name in sc.GN_NONFINITE:
        assert not np.isfinite(np.concatenate([a.ravel() for a in got] + [y.numpy().ravel()])).all(), 'the planted value reached no output'
        if name in ('nan', 'pinf', 'ninf') and relu:                       # the whole (image, group) is NaN, the rest is finite
            bad = np.isnan(y.numpy())
            n, _, ch = sc.BAD_AT
            cpg = sc.GN[name]['C'] // G
            want = np.zeros_like(bad)
            want[n, :, ch // cpg * cpg:(ch // cpg + 1) * cpg] = True
            assert np.array_equal(bad, want)


def test_groupnorm_cases_hold_their_named_features():
    geo = lambda name, dt: sc.gn_geometry(sc.GN[name]['N'], sc.GN[name]['HW'], sc.GN[name]['C'], sc.VE[dt])          # noqa: E731
    assert geo('straddle', 'f32')['dead'] == [4] and geo('straddle', 'bf16')['dead'] == [1]
    for dt in sc.DTYPES:                                                   # every vector of 'straddle' but the first of a 24-channel period holds two groups
        ve, cpg = sc.VE[dt], 6
        assert any(v * ve // cpg != (v * ve + ve - 1) // cpg for v in range(24 // ve))
        assert len(geo('trips', dt)['trips'][0]) > 1, 'row lanes with unequal trip counts'
        assert geo('g-1', dt)['empty'] == 27 and geo('hw-1', dt)['empty'] == 31
    assert sc.GN['g-eq-c']['G'] == sc.GN['g-eq-c']['C'] and sc.GN['g-1']['G'] == 1
    for name, dt in (('chunk2-f32', 'f32'), ('chunk2-bf16', 'bf16')):
        g = geo(name, dt)
        assert g['chunks'] == [256, 1] and g['RL'] == [1, 256] and not g['apply_capped']
    g = geo('cap', 'f32')
    assert g['apply_grid'] == 257 and g['apply_capped'] and g['apply_trips'] == 2
    assert all(not geo(n, dt)['apply_capped'] for n, dt in sc.GN_CASES if n != 'cap')
    c = sc.gn_inputs('offset', 'f32')
    mean, var = ref.gn_stats(c['x'], 4)
    assert (np.abs(mean[:, 1]) > 900 * np.sqrt(var[:, 1])).all() and (np.abs(mean[:, 0]) < 20 * np.sqrt(var[:, 0])).all()
    assert (ref.gn_stats(sc.gn_inputs('zeros', 'f32')['x'], 4)[1] == 0).all()
    assert 99 < np.abs(sc.gn_inputs('wide', 'f32')['x']).max() <= 100
    mean, var = ref.gn_stats(sc.gn_inputs('straddle', 'f32')['x'], 4)      # neighbouring groups: far apart in mean or in scale
    for g0 in range(3):
        assert (np.abs(mean[:, g0] - mean[:, g0 + 1]) > 2 * np.sqrt(np.minimum(var[:, g0], var[:, g0 + 1]))).all() or \
               (np.maximum(var[:, g0], var[:, g0 + 1]) > 3 * np.minimum(var[:, g0], var[:, g0 + 1])).all()
    for kind, test in (('nan', np.isnan), ('pinf', np.isposinf), ('ninf', np.isneginf)):
        for dt in sc.DTYPES:
            assert int(test(sc.gn_inputs(kind, dt)['x']).sum()) == 1
    assert int(np.isnan(sc.gn_inputs('nan-gamma', 'f32')['gamma']).sum()) == 1 and int(np.isnan(sc.gn_inputs('nan-dout', 'bf16')['dout']).sum()) == 1
    for name, dt in sc.GN_CASES:                                           # bf16 cases hold bf16 values
        c = sc.gn_inputs(name, dt)
        assert np.array_equal(sc.rounded(c['x'], dt), c['x'], equal_nan=True) and np.array_equal(sc.rounded(c['dout'], dt), c['dout'], equal_nan=True)
    assert max(np.prod(sc.gn_inputs(n, dt)['x'].shape) for n, dt in sc.GN_CASES) <= 2.5e6


@pytest.mark.parametrize('case', sc.GN_CASES, ids=sc.case_id)
def test_every_pre_activation_keeps_its_margin_from_the_relu_kink(case):
    """at least KINK_MARGIN forward bounds between every finite pre-activation and 0: the kernel's gate (from its own fp32 pre-activation)
    and the reference's are then the same, and no element needs excluding"""
    name, dt = case
    c, g = sc.gn_inputs(name, dt), sc.GN[name]
    n = sc.gn_geometry(g['N'], g['HW'], g['C'], sc.VE[dt])['n']
    _, pre = ref.gn_forward(c['x'], c['gamma'], c['beta'], g['G'], sc.GN_EPS, True)
    bound = ref.gn_forward_bound(c['x'], c['gamma'], c['beta'], g['G'], sc.GN_EPS, n)
    fin = np.isfinite(pre)
    assert fin.any() and (np.abs(pre[fin]) >= ref.KINK_MARGIN * bound[fin]).all()
    assert (pre[fin] > 0).any() and (pre[fin] < 0).any()                   # both sides of the gate occur


def test_groupnorm_bounds_carry_the_statistics_term():
    """the large-offset group's forward bound is dominated by dvar / (2 (var + eps)) and is far larger than its neighbours'; at HW == 1 with
    G == C the reference dx is exactly 0 while its bound (in the magnitudes of the three terms) is not"""
    c = sc.gn_inputs('offset', 'f32')
    n = sc.gn_geometry(2, 35, 24, 4)['n']
    b = ref.gn_forward_bound(c['x'], c['gamma'], c['beta'], 4, sc.GN_EPS, n)
    assert np.median(b[:, :, 6:12] / np.abs(ref.gn_forward(c['x'], c['gamma'], c['beta'], 4, sc.GN_EPS, 0)[1][:, :, 6:12] - c['beta'][6:12])) > 1e-3
    _, drel = ref.gn_stat_errors(c['x'], 4, sc.GN_EPS, n)
    assert 0.01 < drel[0, 0, 6] < 0.25 and drel[0, 0, 0] < 1e-4                 # rstd of the offset group: guaranteed to 20 %, no better
    c = sc.gn_inputs('hw-1-g-eq-c', 'f32')
    dx, _, _ = ref.gn_backward(c['dout'], c['x'], c['gamma'], c['beta'], 8, sc.GN_EPS, 0)
    bdx, _, _ = ref.gn_backward_bounds(c['dout'], c['x'], c['gamma'], c['beta'], 8, sc.GN_EPS, 0, 1)
    assert np.abs(dx).max() < 1e-9 and (bdx > 1e-7).all()


# ------------------------------------------------------------------------------------------ resize
def torch_resize(x, size):
    t = torch.from_numpy(x).double().permute(0, 3, 1, 2).clone().requires_grad_(True)
    return t, F.interpolate(t, size=size, mode='bilinear', align_corners=True)


@pytest.mark.parametrize('name', list(sc.RESIZE))
def test_resize_restatement_equals_torch_float64(name):
    N, ins, outs = sc.RESIZE[name]
    c = sc.resize_inputs(name, 'f32', 1)
    t, y = torch_resize(c['x'], outs)
    y.backward(torch.from_numpy(c['dy']).double().permute(0, 3, 1, 2))
    pin(ref.resize_forward(c['x'], outs)[0], y.permute(0, 2, 3, 1), f'{name} forward')
    want = t.grad.permute(0, 2, 3, 1)
    pin(ref.resize_backward(c['dy'], ins), want, f'{name} transpose')
    tmp, _ = ref.resize_backward_axis(c['dy'], ins[1], 2)                  # W pass then H pass
    pin(ref.resize_backward_axis(tmp, ins[0], 1)[0], want, f'{name} W pass then H pass')
    assert tmp.shape == (N, outs[0], ins[1], c['dy'].shape[3])


def test_resize_cases_hold_their_named_features():
    form = {n: sc.bwd_form(i, o) for n, (_, i, o) in sc.RESIZE.items()}
    assert form == {'x2': 'two-pass', 'x8': 'two-pass', 'identity': '2d', 'mixed': '2d', 'h-in-1': '2d', 'w-in-1': '2d', 'h-out-1': '2d', 'w-out-1': '2d',
                    'down': '2d', 'wide-ratio-2d': '2d', 'long-row': '2d', 'flip': 'two-pass', 'rows-4100': 'two-pass'}
    assert sc.RESIZE['wide-ratio-2d'][2][1] / sc.RESIZE['wide-ratio-2d'][1][1] > 13
    N, _, (Ho, Wo) = sc.RESIZE['rows-4100']
    assert N * Ho > sc.GRID_CAP and all(n * o[0] <= sc.GRID_CAP for k, (n, _, o) in sc.RESIZE.items() if k != 'rows-4100')
    for dt in sc.DTYPES:
        ve = sc.VE[dt]
        assert sc.w_pass_kernel(2400, 3 * ve, ve) == 'global' and sc.w_pass_kernel(2400, ve, ve) == 'lds'
        e = sc.LDS_EDGE
        assert sc.w_pass_kernel(e['Ao'], e['nv'] * ve, ve) == 'global' and sc.w_pass_kernel(e['Ao'], ve, ve) == 'lds'
        assert 0 < e['Ao'] * e['nv'] * 16 - 65536 <= 48
        assert all(sc.w_pass_kernel(o[1], nv * ve, ve) == 'lds' for k, (_, i, o) in sc.RESIZE.items() if form[k] == 'two-pass' for nv in (1, 3))
    # out == 1 and in == 1: scale 0, the full-range branch of dst_range
    assert sc.scale32(4, 1) == 0 and sc.scale32(1, 3) == 0 and sc.dst_range32(0, 1, 3) == (0, 2) and sc.dst_range32(2, 4, 1) == (0, 0)
    # downsizing: inputs that receive no gradient, in float64 and in the kernel's own float32 index arithmetic
    R = ref.resize_axis(16, 8)[0]
    dead = [i for i in range(16) if not R[:, i].any()]
    assert dead == [1, 14] == [i for i in range(16) if not len(sc.contributors32(i, 16, 8))]
    dx = ref.resize_backward(sc.resize_inputs('down', 'f32', 1)['dy'], (16, 16))
    assert (dx[:, dead] == 0).all() and (dx[:, :, dead] == 0).all() and (dx[:, 2:14, 2:14] != 0).all()
    # 'flip': the fp32 source index lands on the other side of an integer (what the bound's neighbour term covers), and beyond in - 1;
    # wherever the fp32 and the float64 index differ, in any case, the restatement has marked the output as near an integer
    for k, (_, i, o) in sc.RESIZE.items():
        for a in (0, 1):
            ax = ref.resize_axis(i[a], o[a])
            assert ax[4][sc.index32(i[a], o[a])[0] != ax[3]].all(), (k, a)
    assert np.nonzero(ref.resize_axis(8, 64)[4])[0].tolist() == [9 * k for k in range(1, 8)] and not ref.resize_axis(4, 1)[4].any()    # x8: s = o / 9; out == 1: never
    assert (sc.index32(3, 42)[0] != ref.resize_axis(3, 42)[3]).any() and sc.scale32(4, 22) * sc.F32(21) > 3
    assert all((sc.index32(i[a], o[a])[0] == ref.resize_axis(i[a], o[a])[3]).all() for k, (_, i, o) in sc.RESIZE.items() if k != 'flip' for a in (0, 1))
    # every contributor lies inside dst_range, even without its margin of one (the margin is pure safety: a kernel without it computes the same)
    for k, (_, i, oo) in sc.RESIZE.items():
        for a in (0, 1):
            for inp in range(i[a]):
                c = sc.contributors32(inp, i[a], oo[a])
                lo, hi = sc.dst_range32(inp, i[a], oo[a], margin=0)
                assert len(c) == 0 or (lo <= c.min() and c.max() <= hi), (k, a, inp)


def test_resize_bound_has_the_weight_term():
    """a constant image is resized exactly: its bound is the blend's roundings alone; a ramp adds ulp(s) |x[i1] - x[i0]|"""
    flat, ramp = np.ones((1, 8, 12, 4)), np.broadcast_to(np.arange(12.0)[None, None, :, None] * 100, (1, 8, 12, 4))
    bf, br = ref.resize_forward(flat, (64, 96))[1], ref.resize_forward(ramp, (64, 96))[1]
    yr = ref.resize_forward(ramp, (64, 96))[0]                                               # the ramp is positive: the blend of |x| is y itself
    sx = ref.resize_axis(12, 96)[2]
    assert np.allclose(bf, 6 * ref.U)
    assert np.allclose(br - 6 * ref.U * yr, ((ref.ULP * sx + ref.U) * 100)[None, None, :, None], rtol=1e-9, atol=0)      # one step of the ramp times ds, on the W axis alone
    assert (br[:, :, 1:] > 6 * ref.U * yr[:, :, 1:] * 1.01).all()


# ------------------------------------------------------------------------------------------ dice
def torch_dice(c):
    nc = c['nc']
    l = torch.from_numpy(c['logits'][..., :nc]).double().clone().requires_grad_(True)                      # [N, HW, nc]
    t = torch.from_numpy(c['targets']).double()                                                           # [N, nc, HW]
    p = torch.softmax(l, 2)
    w = None if c['cw'] is None else [float(v) for v in c['cw']]
    loss = 1 + seg_ref.soft_dice_criterion(p.permute(0, 2, 1)[..., None], t[..., None], w)
    up = 1.0 if c['upstream'] is None else c['upstream']
    (loss * up).backward()
    return p, loss, l.grad


@pytest.mark.parametrize('name', list(sc.DICE) + list(sc.WGRAD))
def test_dice_restatement_equals_torch_float64(name):
    c = sc.dice_inputs(name)
    p, loss, grad = torch_dice(c)
    l = c['logits'][..., :c['nc']]
    up = 1.0 if c['upstream'] is None else c['upstream']
    pin(ref.softmax(l), p, f'{name} softmax')
    pin(np.array(ref.dice_loss(l, c['targets'], c['cw'])), loss, f'{name} loss')
    pin(ref.dice_grad(l, c['targets'], c['cw'], up), grad, f'{name} gradient')


def test_dice_cases_hold_their_named_features():
    for name, c in sc.DICE.items():
        g = sc.dice_geometry(c['H'] * c['W'], c['nc'], c['ld'])
        assert g['maxc'] == (4 if c['nc'] <= 4 else 8 if c['nc'] <= 8 else 32)
        assert g['tail_clamp'] == (c['nc'] <= 8), name                    # every case at nc <= 8 hits the four-in-flight tail clamp
        assert g['bwd_blocks'] < 4096
        assert g['vector'] == (c['nc'] <= 4 and c['ld'] % 4 == 0)
    scalar4 = sorted(k for k, c in sc.DICE.items() if c['nc'] <= 4 and not sc.dice_geometry(c['H'] * c['W'], c['nc'], c['ld'])['vector'])
    assert scalar4 == ['nc1-ld5', 'nc2-ld7', 'nc3-ld6', 'nc4-ld5']       # MAXC == 4 without the 16-byte path: pitches that are no multiple of 4
    assert sc.dice_geometry(37 * 29, 3, 8)['vector'] and sc.dice_geometry(37 * 29, 2, 12)['vector']          # 8 and 12 still take it
    assert {c['nc'] for c in sc.DICE.values()} >= {1, 2, 3, 4, 5, 8, 9, 32}
    assert {c['H'] * c['W'] for c in sc.DICE.values()} >= {1, 63, 65, 1025, 37 * 29}
    for nc in (5, 8, 9, 32):                                               # with and without weights, upstream given and NULL
        cs = [c for c in sc.DICE.values() if c['nc'] == nc]
        assert {c['weights'] for c in cs} == {True, False} and any(c['upstream'] is None for c in cs) and any(c['upstream'] is not None for c in cs)
    for name in ('nc1-ld4', 'nc2-ld4', 'nc3-ld4', 'nc2-ld12', 'nc3-ld8', 'nc3-ld6', 'nc1-ld5', 'nc2-ld7', 'nc4-ld5'):      # garbage padding that would win the max
        c = sc.dice_inputs(name)
        assert c['logits'][..., c['nc']:].min() > np.abs(c['logits'][..., :c['nc']]).max()
    c = sc.dice_inputs('spread80')
    p = ref.softmax(c['logits'][..., :3])
    assert p.min() < 2.0 ** -149 and np.abs(c['logits'][..., :3]).max() > 79
    assert np.abs(sc.dice_inputs('nc3-ld4')['logits'][..., :3]).max() > 11.9
    c = sc.dice_inputs('empty-class')
    assert c['targets'][:, 1].sum() == 0 and c['targets'][:, 0].sum() > 0
    c = sc.dice_inputs('nan')
    assert int(np.isnan(c['logits']).sum()) == 1
    g = ref.dice_grad(c['logits'][..., :3], c['targets'], None, 1.7)
    n = sc.DICE_NAN_AT[0]
    assert np.isnan(g[n]).all() and np.isfinite(np.delete(g, n, 0)).all() and np.isnan(ref.dice_loss(c['logits'][..., :3], c['targets']))
    N, H, W, nc, Wi = sc.WGRAD['rows-4098']
    assert N * H > sc.GRID_CAP and W == 8 and Wi == 2 and all(n * h <= sc.GRID_CAP for k, (n, h, *_) in sc.WGRAD.items() if k != 'rows-4098')


# ------------------------------------------------------------------------------------------ comparers
def _perturbed(refv, bound, factor, seed=0):
    rng = np.random.RandomState(seed)
    return refv + factor * bound * np.where(rng.uniform(size=np.shape(refv)) < 0.5, -1.0, 1.0)


def test_comparers_accept_half_and_reject_twice_their_bound():
    c = sc.gn_inputs('straddle', 'f32')
    n = sc.gn_geometry(2, 35, 24, 4)['n']
    y, _ = ref.gn_forward(c['x'], c['gamma'], c['beta'], 4, sc.GN_EPS, 0)
    dx, dg, db = ref.gn_backward(c['dout'], c['x'], c['gamma'], c['beta'], 4, sc.GN_EPS, 1)
    bdx, bdg, bdb = ref.gn_backward_bounds(c['dout'], c['x'], c['gamma'], c['beta'], 4, sc.GN_EPS, 1, n)
    r = sc.resize_inputs('x2', 'f32', 1)
    ry, rb = ref.resize_forward(r['x'], (10, 14))
    tx, tb = ref.resize_backward(r['dy'], (5, 7)), ref.resize_backward_bound(r['dy'], (5, 7), 'two-pass', False)
    d = sc.dice_inputs('nc3-ld4')
    g = ref.dice_grad(d['logits'][..., :3], d['targets'], d['cw'], 1.7)
    bl, bg = ref.dice_bounds(d['logits'][..., :3], d['targets'], d['cw'], 1.7, 11)
    loss = np.array([ref.dice_loss(d['logits'][..., :3], d['targets'], d['cw'])])
    for refv, bound, what in ((y, ref.finish(ref.gn_forward_bound(c['x'], c['gamma'], c['beta'], 4, sc.GN_EPS, n), y, False), 'gn y'),
                              (y, ref.finish(ref.gn_forward_bound(c['x'], c['gamma'], c['beta'], 4, sc.GN_EPS, n), y, True), 'gn y bf16'),
                              (dx, ref.finish(bdx, dx, False), 'gn dx'), (dg, ref.gn_param_bound(bdg, dg), 'dgamma'), (db, ref.gn_param_bound(bdb, db), 'dbeta'),
                              (ry, ref.finish(rb, ry, False), 'resize'), (tx, ref.finish(tb, tx, True), 'resize transpose'),
                              (g, bg, 'dice gradient'), (loss, np.array([bl]), 'dice loss')):
        assert (bound > 0).all(), what
        assert abs(ref.check(_perturbed(refv, bound, 0.5), refv, bound, what) - 0.5) < 1e-3
        with pytest.raises(AssertionError, match='times the bound'):
            ref.check(_perturbed(refv, bound, 2.0), refv, bound, what)
        one = refv.copy()                                                  # one single element at twice its bound is enough: nothing is averaged
        k = np.unravel_index(one.size // 2, one.shape)
        one[k] += 2.0 * np.broadcast_to(bound, one.shape)[k]
        with pytest.raises(AssertionError, match='times the bound'):
            ref.check(one, refv, bound, what)
    # NaN and infinity patterns must match exactly
    bad = y.copy()
    bad[0, 0, 0] = np.nan
    with pytest.raises(AssertionError, match='NaN mask'):
        ref.check(bad, y, 1.0)
    with pytest.raises(AssertionError, match='NaN mask'):
        ref.check(y, bad, 1.0)
    inf = y.copy()
    inf[0, 0, 0] = np.inf
    with pytest.raises(AssertionError, match='infinities'):
        ref.check(y, inf, 1.0)
    assert ref.check(inf, inf, 1.0) == 0.0 and ref.check(bad, bad, 1.0) == 0.0
