"""csrc/pool.hip driven directly (ops.rec_sppf_pool_fwd / _bwd, rec_upsample_fwd / _bwd, rec_stem_prep, rec_nchw_to_nhwc through ops.run; no
model) on an MI355X against the numpy restatement tests/pool_ref.py, on the cases of tests/pool_cases.py (tests/test_pool_ref_host.py proves
on the CPU that the restatement is ATen's max_pool2d / interpolate / pad / permute, what each case contains and which kernel variant the
launcher must pick for it).

Every SPPF case asserts from the dispatch log that the variant it is listed for ran: forward keys-32 / keys-16 / float-32 / float-16 /
8-channel, each with and without positions (the float-compare bf16 kernels under HDY_SPPF_NO_KEYS), backward 16-channel / 8-channel with two
position planes / with one.  Tensors are channel slices of one buffer (plain, or with 8 channels of 7.0 on either side) between 7.0; the
position tables are cut out of a larger byte buffer; all of it must be intact after each call.  A plane that does not fit raises HdyError
before any launch and leaves every output at its prefill.

Criteria (derivations in pool_ref).  SPPF forward: every element of the three levels equal to the reference in bits (any NaN for a NaN), the
position bytes equal to the reference's under ATen's NaN policy ('last') for the float-compare variants and 'first' for the keys variants; the
keys variants may return +0 where the reference has -0 (documented: the key of -0 is that of +0), nothing else; the inference form gives the
training form's bits.  SPPF backward, from the positions the forward kernel wrote: every element within 33 U A (bf16: half a bf16 ulp on
top), sum(dx) == sum(g0..g3) within the summed bound, two runs equal in bits, exact for integer gradients in fp32.  Upsample forward,
stem_prep and nchw_to_nhwc: bits.  Upsample backward: 5 U A (bf16: half an ulp on top), exact on integers, a NaN prefill fully overwritten
when not accumulating.  No bound comes from a kernel's output and no element is excluded.

Findings.
  * A window holding nothing but -inf lost its gradient at the left and top border.  The float-compare kernels (fp32, bf16 with fp32 planes,
    and the two bf16 float-compare kernels) started each stage at tap 0, which there lies in the 2-pixel border, and the backward never
    gathers from the border: sum(dx) fell short of sum(g) (the 'ninf' families).  ATen starts at the first in-bounds element.  Both stages of
    sppf_pool_fwd_kernel now start at tap max(0, 2 - w) / max(0, 2 - h); the keys kernel needed nothing (the border key 0 lies below the key
    of -inf).  Confirmed and fixed.
  * Keys kernel, signed zeros: a window of -0 alone gives +0 where ATen gives -0; positions follow ATen.  Confirmed, accepted, pinned above.
  * Keys kernel, NaNs: the gradient of a NaN window goes to its first NaN in row-major order, ATen's and the float-compare kernels' to the
    last.  Confirmed, accepted, pinned through the position bytes of the 'nan' families.

Measured on an MI355X, worst case of each group, error in units of its bound (must stay <= 1); in brackets what the same expressions rounded
in fp32 by numpy on the CPU give for the same cases (test_pool_ref_host prints them):

    group (cases)                                    worst error / bound (case)                      median   [CPU fp32]
    SPPF backward fp32, 8 ch. two planes (20)        0.060 (f32-2x12x13x8-pinf-plan)                 0.055    [0.093 worst, 0.057 median,
    SPPF backward fp32, 8 ch. one plane (2)          0.044 (f32-1x40x40x8-random-wide)               0.043     all 22 fp32 cases]
    SPPF backward bf16, 16 channels (28)             0.996 (bf16-2x12x13x32-zeros-wide)              0.994    [0.996 worst, 0.988 median,
    SPPF backward bf16, 8 ch. two planes (16)        0.996 (bf16-2x12x13x8-zeros-wide)               0.985     all 47 bf16 cases]
    SPPF backward bf16, 8 ch. one plane (3)          0.996 (bf16-1x40x40x16-random-plan)             0.991
    upsample backward fp32, store (9)                0.389 (f32-2x5x3x40-pitched)                    0.304    [0.406 worst, 0.317 median,
    upsample backward fp32, accumulate (9)           0.405 (f32-3x6x5x40)                            0.287     store and accumulate]
    upsample backward fp32, NaN / inf (18)           0.412 (f32-3x6x5x40)                            0.280
    upsample backward fp32, above the grid cap (1)   0.646
    upsample backward bf16, store (9)                0.996 (bf16-3x6x5x8-pitched)                    0.996    [0.996 worst, 0.988 median]
    upsample backward bf16, accumulate (9)           0.996 (bf16-3x6x5x8-pitched)                    0.988
    upsample backward bf16, NaN / inf (18)           0.996 (bf16-3x6x5x8-pitched)                    0.988
    integer gradients (SPPF fp32, upsample both)     exact
    SPPF forward (76 cases, 35 of them again under HDY_SPPF_NO_KEYS), upsample forward, stem_prep, nchw_to_nhwc: bits, as stated above

A bf16 result sits near 1 by construction: half a bf16 ulp is nearly all of its bound and some element always rounds that far.  The fp32
figures are far below 1 because the bound counts 33 (5) roundings of the sum of magnitudes and few windows send that many gradients to one
element.  Without the first-in-bounds-tap start the 'ninf_plane' and 'ninf_but_one' cases of every float-compare variant fail on their
position bytes (0x00 for 0x22 at the top-left corner) and on the backward sum; the keys variants pass either way.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import pool_cases as pc  # noqa: E402
import pool_ref as ref  # noqa: E402
from hd_yolo_amd import _lib, ops  # noqa: E402

DEV = torch.device('cuda', 0)
PAD, PREFILL, BYTE = 64, 3.0, 0xA5
TORCH = {'f32': torch.float32, 'bf16': torch.bfloat16}
INT_VIEW = {torch.float32: torch.int32, torch.bfloat16: torch.int16}
CASES = pc.sppf_cases()


def figure(group, what, worst):
    print(f'POOLFIG {group} | {what} | {worst:.3f}')
    return worst


def tbits(t):
    return t.contiguous().view(INT_VIEW[t.dtype])


def host(t):
    return t.float().cpu().numpy()


def dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a)).to(TORCH[dt]).to(DEV)


def logged(recs):
    _lib.dispatch_log(reset=True)
    ops.run(recs)
    torch.cuda.synchronize()
    return _lib.dispatch_log(reset=True)


# ------------------------------------------------------------------------------------------ buffers
class Pitched:
    """[N, H, W, C] as the channel slice at `off` of a pitch off + C + tail buffer between PAD elements, 7.0 everywhere outside the slice"""

    def __init__(self, dt, shape, off=8, tail=8, fill=PREFILL, a=None):
        N, H, W, C = shape
        n = N * H * W * (off + C + tail)
        self.flat = torch.full((n + 2 * PAD,), pc.POISON, dtype=TORCH[dt], device=DEV)
        self.buf = self.flat[PAD:PAD + n].view(N, H, W, off + C + tail)
        self.off, self.C = off, C
        self.v = self.buf[..., off:off + C]
        self.v.copy_(dev(a, dt)) if a is not None else self.v.fill_(fill)
        assert self.v.data_ptr() % 16 == 0

    def slices(self, k):
        c = self.C // k
        return [self.v[..., i * c:(i + 1) * c] for i in range(k)]

    def intact(self):
        ok = (self.flat[:PAD] == pc.POISON).all() and (self.flat[-PAD:] == pc.POISON).all()
        ok = ok and (self.buf[..., :self.off] == pc.POISON).all() and (self.buf[..., self.off + self.C:] == pc.POISON).all()
        assert bool(ok), 'the 7.0 around a tensor was overwritten'


class Tables:
    """three position tables [N, H, W, C] of bytes inside one larger byte buffer"""

    def __init__(self, shape):
        n = int(np.prod(shape))
        m = (n + 15) // 16 * 16
        self.raw = torch.full((3 * (m + PAD) + PAD,), BYTE, dtype=torch.uint8, device=DEV)
        self.t = [self.raw[PAD + k * (m + PAD):PAD + k * (m + PAD) + n].view(shape) for k in range(3)]
        self.out = torch.ones_like(self.raw, dtype=torch.bool)
        for k in range(3):
            self.out[PAD + k * (m + PAD):PAD + k * (m + PAD) + n] = False
        assert all(t.data_ptr() % 16 == 0 for t in self.t)

    def intact(self):
        assert bool((self.raw[self.out] == BYTE).all()), 'bytes around a position table were overwritten'

    def host(self):
        return [t.cpu().numpy() for t in self.t]


def sppf_buffer(dt, shape, layout, x):
    N, H, W, C = shape
    side = 8 if layout == 'wide' else 0
    b = Pitched(dt, (N, H, W, 4 * C), side, side)
    s = b.slices(4)
    s[0].copy_(dev(x, dt))
    return b, s


# ------------------------------------------------------------------------------------------ SPPF forward
def forward(dt, shape, layout, x, positions):
    """-> (the three levels on the host, the device slices, position tables or None, dispatch log)"""
    b, s = sppf_buffer(dt, shape, layout, x)
    tab = Tables(shape) if positions else None
    log = logged([ops.rec_sppf_pool_fwd(s[0], s[1], s[2], s[3], tab.t if positions else None)])
    b.intact()
    assert ref.same_bits(host(s[0]), x, nan_payload=False).all(), 'the input changed'
    if positions:
        tab.intact()
    return [host(t) for t in s[1:]], s, tab, log


def check_forward(dt, shape, layout, fam, positions, no_keys):
    N, H, W, C = shape
    x = pc.family(fam, dt, shape)
    forms = (True, False) if positions else (False,)
    got = {}
    for pos in forms:
        want = pc.fwd_variant(dt, H, W, C, pos, no_keys)
        ys, s, tab, log = forward(dt, shape, layout, x, pos)
        assert log == [want], f'{log} ran, {want} expected'
        keys = 'keys' in want
        rys, _, rpos = ref.sppf_fwd(x, pc.NAN_POLICY[want])
        for lv in range(3):
            ok = ref.same_bits(ys[lv], rys[lv], nan_payload=False, zero_sign=not keys)
            if keys:                                               # the one stated exception: +0 for the reference's -0, never the reverse
                ok &= ~(np.signbit(ys[lv]) & (ys[lv] == 0) & ~np.signbit(rys[lv]))
            assert ok.all(), f'{want} level {lv + 1}: {int((~ok).sum())} elements differ from the reference, first at {np.argwhere(~ok)[0]}'
            if pos:
                p = tab.host()[lv]
                assert np.array_equal(p, rpos[lv]), (f'{want} level {lv + 1}: {int((p != rpos[lv]).sum())} position bytes differ, first at '
                                                     f'{np.argwhere(p != rpos[lv])[0]}: {p[p != rpos[lv]][0]:#x} for {rpos[lv][p != rpos[lv]][0]:#x}')
        got[pos] = [tbits(t).clone() for t in s[1:]]
    if len(forms) == 2:
        assert all(torch.equal(a, b) for a, b in zip(got[True], got[False])), 'the inference form differs from the training form'


KEYED = [c for c in CASES if c[1] == 'bf16' and 'keys' in (pc.fwd_variant(c[1], *c[2][1:], False) or '')]


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_sppf_forward_values_and_positions(case):
    _, dt, shape, fam, layout, positions = case
    check_forward(dt, shape, layout, fam, positions, False)


@pytest.mark.parametrize('case', KEYED, ids=[c[0] for c in KEYED])
def test_sppf_forward_float_compare_kernels_in_bf16(case):
    _, dt, shape, fam, layout, positions = case
    with _lib.option('HDY_SPPF_NO_KEYS', 1):
        check_forward(dt, shape, layout, fam, positions, True)
    assert _lib.load().hdy_get_option(b'HDY_SPPF_NO_KEYS') == 0


@pytest.mark.parametrize('fam', ('random', 'ties', 'zeros', 'nan_window', 'ninf_border'))
def test_sppf_keys_and_float_compare_variants_agree(fam):
    """the same bf16 case through both: equal numbers and NaNs everywhere, equal position bytes outside NaN windows"""
    shape = (2, 12, 13, 32)
    x = pc.family(fam, 'bf16', shape)
    ya, _, ta, la = forward('bf16', shape, 'plan', x, True)
    with _lib.option('HDY_SPPF_NO_KEYS', 1):
        yb, _, tb, lb = forward('bf16', shape, 'plan', x, True)
    assert la == ['sppf_fwd_keys32_pos'] and lb == ['sppf_fwd_float32_pos']
    for lv in range(3):
        assert ref.same_bits(ya[lv], yb[lv], nan_payload=False, zero_sign=False).all()
        keep = ~np.isnan(yb[lv])
        assert np.array_equal(ta.host()[lv][keep], tb.host()[lv][keep])


@pytest.mark.parametrize('dt,shape,positions', pc.REFUSED_FWD, ids=[f'{d}-{"x".join(map(str, s))}-{"pos" if p else "infer"}' for d, s, p in pc.REFUSED_FWD])
def test_sppf_forward_refuses_a_plane_that_does_not_fit(dt, shape, positions):
    x = pc.family('random', dt, shape)
    b, s = sppf_buffer(dt, shape, 'wide', x)
    tab = Tables(shape)
    _lib.dispatch_log(reset=True)
    with pytest.raises(_lib.HdyError, match='does not fit LDS'):
        ops.run([ops.rec_sppf_pool_fwd(s[0], s[1], s[2], s[3], tab.t if positions else None)])
    torch.cuda.synchronize()
    assert _lib.dispatch_log(reset=True) == []
    b.intact()
    assert all(bool((t == PREFILL).all()) for t in s[1:]) and bool((tab.raw == BYTE).all())


# ------------------------------------------------------------------------------------------ SPPF backward
def backward(dt, shape, layout, gs, tab):
    N, H, W, C = shape
    side = 8 if layout == 'wide' else 0
    g = Pitched(dt, (N, H, W, 4 * C), side, side, a=np.concatenate(gs, 3))
    dx = Pitched(dt, shape, fill=float('nan'))
    log = logged([ops.rec_sppf_pool_bwd(*g.slices(4), tab.t, dx.v)])
    g.intact()
    dx.intact()
    tab.intact()
    assert ref.same_bits(host(g.v), np.concatenate(gs, 3)).all(), 'the gradients changed'
    return dx.v, log


TRAINING = [c for c in CASES if c[5]]


@pytest.mark.parametrize('case', TRAINING, ids=[c[0] for c in TRAINING])
def test_sppf_backward_from_the_kernels_own_positions(case):
    name, dt, shape, fam, layout, _ = case
    N, H, W, C = shape
    x = pc.family(fam, dt, shape)
    fwd = pc.fwd_variant(dt, H, W, C, True)
    _, _, tab, log = forward(dt, shape, layout, x, True)
    assert log == [fwd]
    _, idxs, _ = ref.sppf_fwd(x, pc.NAN_POLICY[fwd])
    want_log = [pc.bwd_variant(dt, H, W, C)]
    gs = pc.grads(dt, shape)
    want, A = ref.sppf_bwd(gs, idxs)
    bound = ref.sppf_bwd_bound(A, dt == 'bf16', want)
    d1, log = backward(dt, shape, layout, gs, tab)
    assert log == want_log, f'{log} ran, {want_log} expected'
    got = host(d1).astype(np.float64)
    worst = ref.check(got, want, bound, f'{want_log[0]} after {fwd}')
    total = sum(g.astype(np.float64).sum() for g in gs)
    print(f'POOLSUM {name} | sum(dx) - sum(g) = {got.sum() - total:.3e}, allowed {bound.sum():.3e}')
    assert abs(got.sum() - total) <= bound.sum(), f'sum(dx) = {got.sum()!r}, sum(g0..g3) = {total!r}: a gradient was lost'
    d2, _ = backward(dt, shape, layout, gs, tab)
    assert torch.equal(tbits(d1), tbits(d2)), 'two runs differ'
    figure(f'sppf backward {dt} {want_log[0]}', name, worst)
    if dt == 'f32':
        gi = pc.grads(dt, shape, integer=True)
        wi, Ai = ref.sppf_bwd(gi, idxs)
        assert Ai.max() < 2 ** 24
        di, _ = backward(dt, shape, layout, gi, tab)
        assert np.array_equal(host(di).astype(np.float64), wi), 'integer gradients: not exact'


@pytest.mark.parametrize('dt,shape', pc.REFUSED_BWD, ids=[f'{d}-{"x".join(map(str, s))}' for d, s in pc.REFUSED_BWD])
def test_sppf_backward_refuses_a_plane_that_does_not_fit(dt, shape):
    N, H, W, C = shape
    g = Pitched(dt, (N, H, W, 4 * C), a=np.concatenate(pc.grads(dt, shape), 3))
    dx = Pitched(dt, shape)
    tab = Tables(shape)
    _lib.dispatch_log(reset=True)
    with pytest.raises(_lib.HdyError, match='does not fit LDS'):
        ops.run([ops.rec_sppf_pool_bwd(*g.slices(4), tab.t, dx.v)])
    torch.cuda.synchronize()
    assert _lib.dispatch_log(reset=True) == []
    dx.intact()
    assert bool((dx.v == PREFILL).all())


# ------------------------------------------------------------------------------------------ upsample
def side(pitched):
    return (8, 8) if pitched else (0, 0)


def upsample_forward(dt, shape, pitched, x):
    N, H, W, C = shape
    src = Pitched(dt, shape, *side(pitched), a=x)
    dst = Pitched(dt, (N, 2 * H, 2 * W, C), *side(pitched))
    ops.run([ops.rec_upsample_fwd(src.v, dst.v)])
    torch.cuda.synchronize()
    src.intact()
    dst.intact()
    want = dev(ref.upsample_fwd(x), dt)
    assert torch.equal(tbits(src.v), tbits(dev(x, dt))) and torch.equal(tbits(dst.v), tbits(want)), 'upsample forward: bits differ'


def upsample_backward(dt, shape, pitched, dy, old, group, name):
    N, H, W, C = shape
    src = Pitched(dt, (N, 2 * H, 2 * W, C), *side(pitched), a=dy)
    dst = Pitched(dt, shape, *side(pitched), fill=float('nan'), a=old)
    ops.run([ops.rec_upsample_bwd(src.v, dst.v, accumulate=old is not None)])
    torch.cuda.synchronize()
    src.intact()
    dst.intact()
    assert torch.equal(tbits(src.v), tbits(dev(dy, dt)))
    want, A = ref.upsample_bwd(dy, old)
    return figure(group, name, ref.check(host(dst.v), want, ref.upsample_bwd_bound(A, dt == 'bf16', want), name)), host(dst.v), want


@pytest.mark.parametrize('case', pc.upsample_cases(), ids=[c[0] for c in pc.upsample_cases()])
def test_upsample_forward_and_backward(case):
    name, dt, shape, pitched = case
    N, H, W, C = shape
    big = (N, 2 * H, 2 * W, C)
    upsample_forward(dt, shape, pitched, pc.up_input(dt, shape, 1))
    upsample_forward(dt, shape, pitched, pc.up_input(dt, shape, 2, special=True))
    dy, old = pc.up_input(dt, big, 3), pc.up_input(dt, shape, 4)
    upsample_backward(dt, shape, pitched, dy, None, f'upsample backward {dt} store', name)
    upsample_backward(dt, shape, pitched, dy, old, f'upsample backward {dt} accumulate', name)
    upsample_backward(dt, shape, pitched, pc.up_input(dt, big, 5, special=True), None, f'upsample backward {dt} nonfinite', name)
    upsample_backward(dt, shape, pitched, pc.up_input(dt, big, 6, special=True), pc.up_input(dt, shape, 7, special=True), f'upsample backward {dt} nonfinite', name)
    for o in (None, pc.up_input(dt, shape, 9, integer=True)):
        _, got, want = upsample_backward(dt, shape, pitched, pc.up_input(dt, big, 8, integer=True), o, f'upsample backward {dt} integer', name)
        assert np.array_equal(got.astype(np.float64), want), 'integer gradients: not exact'


def test_upsample_forward_above_the_grid_cap():
    dt, shape = pc.UP_BIG_FWD
    assert pc.up_vectors(dt, shape, True) > pc.GRID_CAP
    upsample_forward(dt, shape, False, pc.up_input(dt, shape, 11))


def test_upsample_backward_above_the_grid_cap():
    dt, shape = pc.UP_BIG_BWD
    N, H, W, C = shape
    assert pc.up_vectors(dt, shape, False) > pc.GRID_CAP
    upsample_backward(dt, shape, False, pc.up_input(dt, (N, 2 * H, 2 * W, C), 12), pc.up_input(dt, shape, 13), f'upsample backward {dt} above the cap', 'accumulate')


# ------------------------------------------------------------------------------------------ stem_prep, nchw_to_nhwc
def stem(dt, B, H, W, pad):
    img = pc.image((B, 3, H, W), H + pad)
    out = Pitched(dt, (B, H + 2 * pad, W + 2 * pad, 4), 0, 0)
    src = torch.from_numpy(img).to(DEV)
    ops.run([ops.rec_stem_prep(src, out.v, pad)])
    torch.cuda.synchronize()
    out.intact()
    ok = ref.same_bits(host(out.v), ref.stem_prep(img, pad, dt), nan_payload=dt == 'f32')
    assert ok.all() and ref.same_bits(src.cpu().numpy(), img).all(), f'stem_prep: {int((~ok).sum())} elements differ'


@pytest.mark.parametrize('dt', pc.DTYPES)
@pytest.mark.parametrize('B,H,W,pad', pc.STEM + [pc.STEM_BIG], ids=['x'.join(map(str, s)) for s in pc.STEM + [pc.STEM_BIG]])
def test_stem_prep_is_pad_and_cast(B, H, W, pad, dt):
    stem(dt, B, H, W, pad)


@pytest.mark.parametrize('dt', pc.DTYPES)
@pytest.mark.parametrize('C', pc.LAYOUT_C)
def test_nchw_to_nhwc_is_permute_and_cast(C, dt):
    for k, (H, W) in enumerate(pc.LAYOUT_HW):
        N = 1 + (k + C) % 3
        srch = pc.image((N, C, H, W), C + k)
        for off, tail in ((0, 0), (8, 3)):
            dst = Pitched(dt, (N, H, W, C), off, tail)
            src = torch.from_numpy(srch).to(DEV)
            ops.run([ops.rec_nchw_to_nhwc(src, dst.v)])
            torch.cuda.synchronize()
            dst.intact()
            ok = ref.same_bits(host(dst.v), ref.nchw_to_nhwc(srch, dt), nan_payload=dt == 'f32')
            assert ok.all() and ref.same_bits(src.cpu().numpy(), srch).all(), f'nchw_to_nhwc C={C} HW={H * W}: {int((~ok).sum())} elements differ'
