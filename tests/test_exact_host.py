"""CPU side of the exact convolution tests (tests/exact_ref.py): the preconditions of the integer-operand recipe
hold for every convolution shape of the parity tests and for every call form of tests/test_gpu_exact_forms.py (exact_ref.FORM_CASES), and the comparer rejects — with the right coordinates — the errors the parity tests' criterion
(`assert_close` with TOL[bf16] = 1.5e-2 of the tensor's maximum, 1e-3 of the largest BatchNorm sum) lets through.  Every shape is checked
(about 20 s of float64 convolutions in all); none is left out."""
import re

import pytest
import torch
import torch.nn.functional as F

import exact_ref as X
from test_gpu_kernels import TOL, assert_close, q, rnd

BF16 = torch.bfloat16
SHAPES = X.all_shapes()


@pytest.mark.parametrize('case,stem', SHAPES, ids=['x'.join(map(str, c)) + ('-stem' if s else '') for c, s in SHAPES])
def test_preconditions_hold(case, stem):
    e = X.reference(case, stem)
    r = X.check_preconditions(e)
    assert r['distinct'] >= 32, f'{case}: only {r["distinct"]} distinct output values'
    # no output lane can be all zero either: a kernel that skipped a filter row would otherwise pass
    assert (e.y.abs().amax((0, 2, 3)) > 0).all()
    # every leg's reference fits its compared type without loss (bf16 is the narrow one)
    for t in (e.y, e.affine + e.acc, e.affine + e.res, F.relu(e.affine)):
        X.lossless(t, BF16)
    if not stem:
        X.lossless(e.dx + e.dx_acc, BF16)
    X.lossless(e.dw + 2.0, torch.float32)


def test_the_shape_lists_are_the_parity_tests_own():
    """the very list objects of tests/test_gpu_kernels.py and the parameters of its stem tests, not copies that could fall behind"""
    import test_gpu_kernels as tk
    conv, deep, wdeep, res, stem, patch = X.case_lists()
    assert conv is tk.CONV_CASES and deep is tk.DEEP_CASES and wdeep is tk.WGRAD_DEEP_CASES and res is tk.RES_CASES
    marks = {m.args[0]: list(m.args[1]) for fn in (tk.test_stem_conv, tk.test_stem_patch_kernel_bf16) for m in fn.pytestmark if m.name == 'parametrize'}
    assert stem == marks['shape'] and [s[3] for s in patch] == marks['K'] and all(s[:3] == (3, 64, 192) for s in patch)
    every = {c for c, _ in SHAPES}
    assert all(c in every for c in list(conv) + list(deep) + list(wdeep)) and all(X.stem_case(*s) in every for s in stem + patch)


def rejected(fn):
    """the AssertionError text of fn(), or None if it passes"""
    try:
        fn()
    except AssertionError as err:
        return str(err)
    return None


def old_accepts(got, ref, tol, what):
    return rejected(lambda: assert_close(got.float(), ref.float(), tol, what)) is None


CASE = (2, 16, 32, 64, 64, 3, 1, 1)          # C = 64, 3x3, the filter-resident kernel's shape: one product term (<= 2) against a maximum of ~70


def test_one_element_off_by_one():
    e = X.reference(CASE)
    ref = X.nhwc(e.y)
    got = ref.to(BF16)
    assert rejected(lambda: X.assert_exact(got, ref, 'y')) is None
    got[1, 9, 17, 42] += 1
    msg = rejected(lambda: X.assert_exact(got, ref, 'y'))
    assert msg and '1 of ' in msg and 'n 1..1, y 9..9, x 17..17, channel 42..42' in msg and '(1, 9, 17, 42): got' in msg, msg
    assert old_accepts(got, ref, TOL[BF16], 'y'), 'the gap this closes: the parity criterion does not see one element off by one'


def test_one_product_term_dropped_at_a_border_pixel():
    """With the integer operands a product term is 1 or 2 against an allowance of 1.5e-2 x max |y| = 1.1: the parity criterion happens to
    reject this term of 2 (asserted as measured).  On the parity tests' own real operands the same term is accepted (asserted below): that is
    where the criterion is blind."""
    e = X.reference(CASE)
    ref = X.nhwc(e.y)
    got = ref.to(BF16)
    n, h, w_, k = 0, 0, 5, 7                     # top border row
    r, s = 1, 2                                  # a tap inside the image there
    c = next(c for c in range(64) if e.w[k, c, r, s] != 0 and e.x[n, c, h + r - 1, w_ + s - 1] != 0)
    got[n, h, w_, k] -= (e.w[k, c, r, s] * e.x[n, c, h + r - 1, w_ + s - 1]).to(BF16)
    msg = rejected(lambda: X.assert_exact(got, ref, 'y'))
    assert msg and '1 of ' in msg and 'n 0..0, y 0..0, x 5..5, channel 7..7' in msg, msg
    assert abs(e.w[k, c, r, s] * e.x[n, c, h + r - 1, w_ + s - 1]) == 2
    assert not old_accepts(got, ref, TOL[BF16], 'y')
    # the same dropped term with conv_case's operands: x ~ U(-1, 1), w ~ U(-1, 1) sqrt(3 / 576), both rounded to bf16
    xr = q(rnd((2, 64, 16, 32), 1), BF16)
    wr = q(rnd((64, 64, 3, 3), 2, (3.0 / 576) ** 0.5), BF16)
    ref_r = F.conv2d(xr, wr, None, 1, 1)
    got_r = ref_r.clone()
    got_r[n, k, h, w_] -= wr[k, c, r, s] * xr[n, c, h + r - 1, w_ + s - 1]
    assert got_r[n, k, h, w_] != ref_r[n, k, h, w_]
    assert old_accepts(got_r, ref_r, TOL[BF16], 'y'), 'the gap this closes: the parity criterion does not see a dropped product term'


def test_one_chunk_of_eight_channels_swapped_between_neighbouring_pixels_under_one_tap():
    """With the integer operands the swap moves an output by up to ~10 against an allowance of 1.1, so the parity criterion rejects it too
    (asserted as measured); with real operands it is a change of ~0.08 against 0.037, caught only sometimes."""
    e = X.reference(CASE)
    ref = X.nhwc(e.y)
    n, h, w_, r, s, c0 = 1, 8, 16, 0, 1, 24      # outputs (8, 16) and (8, 17) read, under tap (0, 1), each other's channels 24..31
    xa, xb = e.x[n, c0:c0 + 8, h + r - 1, w_ + s - 1], e.x[n, c0:c0 + 8, h + r - 1, w_ + 1 + s - 1]
    delta = (e.w[:, c0:c0 + 8, r, s] * (xb - xa)).sum(1)                  # what pixel (h, w_) gains per output channel; its neighbour loses it
    got = ref.clone()
    got[n, h, w_] += delta
    got[n, h, w_ + 1] -= delta
    got = got.to(BF16)
    wrong = (delta != 0).nonzero().flatten()
    assert len(wrong) > 0
    msg = rejected(lambda: X.assert_exact(got, ref, 'y'))
    assert msg and f'{2 * len(wrong)} of ' in msg and f'n 1..1, y 8..8, x 16..17, channel {wrong.min()}..{wrong.max()}' in msg, msg
    assert not old_accepts(got, ref, TOL[BF16], 'y')


def test_one_pixel_added_twice_into_a_statistics_slab():
    """5 x 128 x 128 (81 920 pixels per channel), one slab per 128 pixels as the generic kernel writes them; the double-counted pixels are
    those of row 64 of image 2, a band seam of the band-split kernels.  The exact comparison rejects every one of them and names the slab.

    What the 1e-3 criterion makes of them.  This test was planned to assert that the old criterion ACCEPTS a pixel counted twice; that
    expectation was false and the test asserts what was measured instead.  SUM y is a zero-mean random walk (largest sum ~6000 against
    |y| up to ~50 at one pixel: a median ratio of 3.7e-3, and 2.6e-3 with the parity tests' real operands), so a pixel doubled in all 32
    channels at once trips the 1e-3 bound in some channel: the old criterion REJECTS it at every one of the 128 pixels (asserted).  The
    gap for statistics is therefore narrower than a whole pixel: the sum-of-squares row is off by at most ~2.5e-4 of the largest sum and is
    accepted at every pixel — SUM y^2 cannot reveal a miscount at all — and a double count confined to one channel (one lane's column of
    a tile) is accepted in both rows at 59 of the 128 pixels (both asserted)."""
    case = (5, 128, 128, 32, 32, 3, 1, 1)
    e = X.reference(case)
    K = 32
    rows = X.nhwc(e.y).reshape(-1, K)
    slabs = torch.stack([rows.reshape(-1, 128, K).sum(1), (rows * rows).reshape(-1, 128, K).sum(1)], 1).float()        # [640][2][K]
    ref_slabs = slabs.double()
    assert rejected(lambda: X.assert_stats_exact(slabs, e, 'stats')) is None
    X.assert_exact(slabs, ref_slabs, 'slabs', X.AXES_STAT)

    def doubled(p, channels=slice(None)):
        s = slabs.clone()
        s[p // 128, 0, channels] += rows[p, channels].float()
        s[p // 128, 1, channels] += (rows[p, channels] * rows[p, channels]).float()
        return s

    row = [(2 * 128 + 64) * 128 + i for i in range(128)]
    k1 = 5
    sumsq_ok = [p for p in row if old_accepts(doubled(p).sum(0)[1], e.sumsq, 1e-3, 'stats sumsq')]
    sum_ok = [p for p in row if old_accepts(doubled(p).sum(0)[0], e.sum, 1e-3, 'stats sum')]
    lane_ok = [p for p in row if rows[p, k1] != 0 and old_accepts(doubled(p, k1).sum(0)[0], e.sum, 1e-3, 'stats sum')
               and old_accepts(doubled(p, k1).sum(0)[1], e.sumsq, 1e-3, 'stats sumsq')]
    print(f'of the {len(row)} pixels of the seam row, the 1e-3 criterion accepts a double count: {len(sumsq_ok)} in the SUM y^2 row, {len(sum_ok)} in the '
          f'SUM y row, {len(lane_ok)} (both rows) when only channel {k1} is miscounted')
    assert not sum_ok, 'as measured: a pixel doubled in every channel moves SUM y beyond 1e-3 of the largest sum in some channel'
    assert len(lane_ok) == 59, 'as measured'
    assert len(sumsq_ok) == len(row), 'the gap this closes: SUM y^2 within 1e-3 does not see a pixel counted twice'
    assert lane_ok, 'the gap this closes: the 1e-3 criterion does not see a pixel counted twice in one channel'
    for p in row:
        assert rejected(lambda: X.assert_stats_exact(doubled(p), e, 'stats')) is not None
    for p in lane_ok:
        assert rejected(lambda: X.assert_stats_exact(doubled(p, k1), e, 'stats')) is not None
    p = row[0]
    bad = doubled(p)
    msg = rejected(lambda: X.assert_exact(bad, ref_slabs, 'slabs', X.AXES_STAT))
    nz = (rows[p] != 0).nonzero().flatten()
    assert msg and f'{2 * len(nz)} of ' in msg and f'slab {p // 128}..{p // 128}, stat 0..1, k {nz.min()}..{nz.max()}' in msg, msg
    msg = rejected(lambda: X.assert_stats_exact(bad, e, 'stats'))
    assert msg and re.search(r'slab 0\.\.0, stat 0\.\.1', msg), msg
    msg = rejected(lambda: X.assert_exact(doubled(lane_ok[0], k1), ref_slabs, 'slabs', X.AXES_STAT))
    assert msg and '2 of ' in msg and f'slab {lane_ok[0] // 128}..{lane_ok[0] // 128}, stat 0..1, k {k1}..{k1}' in msg, msg


def test_every_form_case_is_among_the_checked_shapes():
    every = {c for c, _ in SHAPES}
    groups = (X.RAGGED_CASES, X.DECONV_CASES, X.WINDOW_CASES, X.WINDOW_FWD_WGRAD_CASES, X.WINDOW_F32_CASES, X.DECLINED_CASES, [X.REFUSED_WINDOW_CASE, X.DEEP_CONTROL_CASE, X.DESCENDING_DEEP_CASE])
    assert all(len(c) == 9 and c in every and c in X.FORM_CASES for g in groups for c in g)
    assert X.window((2, 20, 20, 64, 32, 1, 1, 0)) == (2, 20, 20, 64, 32, 1, 1, 1, 0)
    e, sq = X.reference((1, 6, 6, 8, 8, 3, 3, 1, 1)), X.reference((1, 6, 6, 8, 8, 3, 1, 1))
    assert torch.equal(e.w, sq.w) and torch.equal(e.y, sq.y), 'a square window stated with 9 numbers is the case stated with 8'
    assert X.uncovered((1, 11, 7, 16, 24, 2, 2, 2, 0)) == (10, 6) and X.uncovered((1, 13, 11, 32, 32, 3, 3, 2, 0)) == (13, 11)


def test_one_tap_of_a_5x5_window_dropped():
    case = (1, 12, 12, 16, 16, 5, 5, 1, 2)
    e = X.reference(case)
    ref = X.nhwc(e.y)
    assert rejected(lambda: X.assert_exact(ref.to(BF16), ref, 'y')) is None
    for r, s in ((0, 0), (2, 2), (4, 3)):                        # a corner tap (inside the image for interior pixels only), the centre, any other
        w = e.w.clone()
        assert w[:, :, r, s].abs().sum() > 0
        w[:, :, r, s] = 0
        got = X.nhwc(F.conv2d(e.x, w, None, 1, 2)).to(BF16)
        msg = rejected(lambda: X.assert_exact(got, ref, 'y'))
        assert msg and ' elements differ' in msg, (r, s)
    # ... and a single product term of one tap at one pixel
    k, c = next((k, c) for k in range(16) for c in range(16) if e.w[k, c, 4, 3] != 0 and e.x[0, c, 5 + 4 - 2, 6 + 3 - 2] != 0)
    got = ref.to(BF16)
    got[0, 5, 6, k] -= (e.w[k, c, 4, 3] * e.x[0, c, 7, 7]).to(BF16)
    msg = rejected(lambda: X.assert_exact(got, ref, 'y'))
    assert msg and '1 of ' in msg and f'n 0..0, y 5..5, x 6..6, channel {k}..{k}' in msg, msg


def test_nonzero_row_behind_k_in_a_padded_weight_gradient():
    """K = 27 padded to 32: rows 27 .. 31 of the gradient are zero, and one value there — what a kernel that did not mask its zero channels,
    or a reduction that read a row too far, would leave — is named"""
    e = X.reference((2, 20, 20, 128, 27, 1, 1, 1, 0))
    ref = torch.cat([e.dw, torch.zeros((5, 128, 1, 1), dtype=torch.float64)])
    got = ref.float()
    assert rejected(lambda: X.assert_exact(got, ref, 'dw', X.AXES_W)) is None
    got[27, 100, 0, 0] = 1.0
    msg = rejected(lambda: X.assert_exact(got, ref, 'dw', X.AXES_W))
    assert msg and '1 of ' in msg and 'k 27..27, c 100..100, r 0..0, s 0..0' in msg, msg
    got = ref.float()
    got[31] = float('nan')                                       # a row the call never wrote
    msg = rejected(lambda: X.assert_exact(got, ref, 'dw', X.AXES_W))
    assert msg and '128 of ' in msg and 'k 31..31' in msg, msg


def test_changed_guard_lane_of_a_channel_slice():
    """K = 27 in lanes 1 .. 28 of a 30-lane buffer: the lane in front of the slice, the first lane behind it (where a vector store of the last
    whole group of channels would land) and the slice itself are all under the one comparison"""
    e = X.reference((2, 20, 20, 128, 27, 1, 1, 1, 0))
    want = X.in_slice(X.nhwc(e.y), 30, 1, 5.0)
    assert want.shape == (2, 20, 20, 30) and (want[..., 0] == 5.0).all() and (want[..., 28:] == 5.0).all() and torch.equal(want[..., 1:28], X.nhwc(e.y))
    got = want.float()
    assert rejected(lambda: X.assert_exact(got, want, 'y')) is None
    for lane in (0, 28, 29):
        bad = got.clone()
        bad[1, 19, 19, lane] = 0.0
        msg = rejected(lambda: X.assert_exact(bad, want, 'y'))
        assert msg and '1 of ' in msg and f'n 1..1, y 19..19, x 19..19, channel {lane}..{lane}' in msg and 'got 0.0 want 5.0' in msg, msg
    # an fp32 result rounded through bf16 on its way out: 301 becomes 302
    big = X.nhwc(e.y + 301.0)
    assert rejected(lambda: X.assert_exact(big.float(), big, 'y')) is None
    assert ' elements differ' in rejected(lambda: X.assert_exact(big.to(BF16).float(), big, 'y'))


def test_comparer_sees_nan_and_shape_and_inexact_references():
    ref = torch.arange(24.0, dtype=torch.float64).reshape(1, 2, 3, 4)
    got = ref.to(BF16)
    got[0, 1, 2, 3] = float('nan')
    assert 'y 1..1, x 2..2, channel 3..3' in rejected(lambda: X.assert_exact(got, ref, 'nan'))
    assert 'shape' in rejected(lambda: X.assert_exact(got[:, :1], ref, 'shape'))
    assert 'exactly' in rejected(lambda: X.assert_exact(got, ref + 257.0, 'inexact'))          # 257 + odd values need nine bits
    X.assert_exact(torch.tensor([-0.0]), torch.tensor([0.0], dtype=torch.float64), 'zeros', ('i',))
    slabs = torch.zeros((3, 2, 4))
    slabs[1, 0, 2] = float('nan')

    class E:
        sum = sumsq = torch.zeros(4, dtype=torch.float64)
    assert 'slabs hold a non-finite value, the first ones [1]' in rejected(lambda: X.assert_stats_exact(slabs, E, 'poison'))


def test_bf16_ulp_measure():
    b = torch.tensor([1.0, 1.0, 0.0, 100.0])
    a = torch.tensor([1.0 + 2.0 ** -7, 1.0 + 2.0 ** -6, 2.0 ** -17, 100.0])
    assert X.ulps_bf16(a, b).tolist() == [1.0, 2.0, 1.0, 0.0]
