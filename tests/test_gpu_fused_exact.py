"""The fused 1x1 backward (csrc/conv1x1_bwd.hip, instances 32 / 64 / 96 / 128) and the two producers of BatchNorm-backward statistics
(hdy_conv1x1_bwd_fused_stats, hdy_conv_dgrad_stats with the igemm_128x{32,64}x2[_walk]_stat instances) on an MI355X against
tests/fused_ref.py: integer operands for which dx, dW and every slab are exact, so the comparison is equality with a float64 reference and
a mismatch is reported with its (row, channel), (k, c) or (slab, stat, channel); and real-valued operands through an identity filter, where
dx is the kernel's dy and is held to the per-element criterion of the apply pass.  tests/test_fused_ref_host.py proves on the CPU what every
case contains and that the comparers reject the errors this data movement can make.

Buffers: every operand is a channel slice of a wider buffer at a nonzero multiple-of-8 offset, each with its own pitch, 7.0 outside; dx is
NaN where the call only writes and dx0 where it accumulates; the gradients, the weight-gradient workspace (plus one float that must stay NaN)
and the statistics slabs (plus one slab that must stay NaN) are NaN-filled.  After each launch the 7.0 outside every slice is intact.

Probe (first test): K = 64, M = 130, W = identity, c1 = c2 = 0, scale 1, saturated shift: dx equals dz bit for bit, so v_rcp_f32(1.0f) is
1.0f on this device and silu'(u >= 24) evaluates to exactly 1.  Measured on an MI355X: it holds (dx == dz in all 130 x 64 elements), so no exact leg is skipped.

Paths reached (fused_ref.geometry, asserted against the library's queries, and the dispatch log):
    conv1x1_bwd_32 / _64    M = 1, 127, 128, 129, 421 (1 tile per workgroup), 65669 (2 tiles, both x buffers, 255 workgroups without tiles,
                            5 rows in the last tile), 131205 (3 tiles: buffer 0 reused, 170 workgroups without tiles); statistics requests
                            whole / split at 8 / inner (first and last chunk unserved) at M = 129, 65669, 131205, written and accumulated
    conv1x1_bwd_96 / _128   M = 1, 63, 64, 65, 229, 32837 (2 tiles), 65605 (3 tiles; the 128-wide instance refills its single x buffer)
    igemm_128x64x2_stat     1x1 into 64 channels (8 tiles), 98437 pixels (770 tiles on 768 workgroups: 2 tiles, 383 without tiles)
    igemm_128x32x2_stat     3x3 into 32 channels (6 tiles), 131205 pixels (1026 tiles on 1024 workgroups: 2 tiles, 511 without tiles)
    igemm_128x64x2_walk_stat  3x3 / stride 2 into 64 channels: 2 m-tiles x 4 parity classes

Found by these tests: a workgroup of an igemm statistics instance that had no tile returned before writing its slab, so the slabs of
hdy_conv_dgrad_stats were only complete over a zeroed array (the two long cases: 383 and 511 slabs stayed NaN).  It now writes zeros.

Measured on an MI355X, worst error in units of its bound (must stay <= 1):
    group (cases)                            worst error / bound (case)                  others
    probe                                    dx == dz bit for bit: v_rcp_f32(1.0f) == 1.0f
    exact legs (28 + 18 + 15)                equality; nothing to measure
    elementwise, identity filter (16)        0.968 (64-129)                              0.943 to 0.964; the same with dz in one tensor or two
    SiLU statistics, sums (3)                0.011 (igemm_128x64x2_walk_stat)            fused 64: 0.004, igemm_128x32x2_stat: 0.008
    SiLU statistics, finalize of slabs (3)   0.977 (igemm_128x64x2_walk_stat)            fused 64: 0.893, igemm_128x32x2_stat: 0.897

A bf16 output sits near 0.97 by construction (half a bf16 ulp is 2^-8 / (2^-8 + 1e-4) of its bound), and a finalize output near 1: its
bound is the one fp32 rounding of the result.  The yardstick c of the SiLU sums was 5.4 to 5.7; the chains are
40 (fused 64, two tiles), 66 (bn 32) and 36 (bn 64) additions.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bn_cases as bc  # noqa: E402
import bn_ref  # noqa: E402
import exact_ref as X  # noqa: E402
import fused_ref as F  # noqa: E402
from hd_yolo_amd import _lib, ops  # noqa: E402

DEV = torch.device('cuda', 0)
BF16 = torch.bfloat16
NAN = float('nan')
PAD = 4                                            # floats around a parameter vector (16 bytes: the requests' coefficients stay aligned)


def figure(group, what, worst):
    print(f'F1FIG {group} | {what} | {worst:.3f}')
    return worst


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64))


# ------------------------------------------------------------------------------------------ buffers
class Rows:
    """an [M, K] array as the NHWC bf16 view [N, H, W, K] (default [1, 1, M, K]) at channel `off` of a pitch K + off + tail buffer, 7.0
    everywhere else; a=None: the view is filled with `fill` (an output's prefill)"""

    def __init__(self, a, K=None, M=None, off=8, tail=8, fill=NAN, nhw=None):
        M, K = a.shape if a is not None else (M, K)
        n, h, w = nhw or (1, 1, M)
        assert n * h * w == M and off % 8 == 0 and tail % 8 == 0 and off > 0
        self.K, self.M, self.off = K, M, off
        self.buf = torch.full((n, h, w, K + off + tail), bc.POISON, dtype=BF16, device=DEV)
        self.v = self.buf[..., off:off + K]
        if a is not None:
            self.v.copy_((t64(a) if isinstance(a, np.ndarray) else a).to(BF16).view(n, h, w, K))
        else:
            self.v.fill_(fill)

    def flat(self):
        return self.v.reshape(self.M, self.K)

    def host(self):
        return self.flat().float().cpu().numpy().astype(np.float64)

    def intact(self):
        assert (self.buf[..., :self.off] == bc.POISON).all() and (self.buf[..., self.off + self.K:] == bc.POISON).all(), 'poison outside the view overwritten'


class Vec:
    """a per-channel fp32 vector in the middle of a 7.0-filled buffer"""

    def __init__(self, a=None, K=None, fill=NAN):
        K = len(a) if a is not None else K
        self.K = K
        self.buf = torch.full((K + 2 * PAD,), bc.POISON, dtype=torch.float32, device=DEV)
        self.v = self.buf[PAD:PAD + K]
        if a is not None:
            self.v.copy_(torch.from_numpy(np.ascontiguousarray(a, np.float32)))
        else:
            self.v.fill_(fill)

    def host(self):
        return self.v.cpu().numpy().astype(np.float64)

    def intact(self):
        assert (self.buf[:PAD] == bc.POISON).all() and (self.buf[PAD + self.K:] == bc.POISON).all(), 'poison around a vector overwritten'


class Guarded:
    """`n` leading elements (rows) NaN-filled, one more behind them that must still be NaN after the launch"""

    def __init__(self, n, *shape):
        self.buf = torch.full((n + 1,) + shape, NAN, dtype=torch.float32, device=DEV)
        self.v = self.buf[:n]

    def intact(self, what):
        assert torch.isnan(self.buf[-1]).all(), f'{what}: written past its end'


class Grads:
    """dW as K rows of a [K + 2][C][1][1] buffer: NaN inside, a row of 7.0 before and after; split into (grad_a, grad_b)"""

    def __init__(self, K, C, split):
        self.buf = torch.full((K + 2, C, 1, 1), bc.POISON, dtype=torch.float32, device=DEV)
        self.v = self.buf[1:K + 1]
        self.v.fill_(NAN)
        ka, kb = split
        self.a, self.b = self.v[:ka], (self.v[ka:ka + kb] if kb else None)
        self.rows = ka + kb

    def intact(self):
        assert (self.buf[0] == bc.POISON).all() and (self.buf[-1] == bc.POISON).all(), 'poison around the weight gradient overwritten'


def launch(records):
    _lib.dispatch_log(reset=True)
    ops.run(records)
    torch.cuda.synchronize()
    return _lib.dispatch_log(reset=True)


def pack_dgrad(w_kc, R=1, stride=1, pad=0):
    """w [K][C][R][R] float64 -> the packed data-gradient filter"""
    w = (t64(w_kc) if isinstance(w_kc, np.ndarray) else w_kc.double()).float()
    if w.dim() == 2:
        w = w[:, :, None, None]
    K, C = w.shape[:2]
    wpd = ops.pack_alloc(K, C, R, R, stride, pad, ops.PACK_DGRAD, BF16, DEV).fill_(NAN)
    ops.run([ops.rec_pack(w.contiguous().to(DEV), None, stride, pad, ops.PACK_DGRAD, wpd)])
    return wpd


def equal_or_explain(got, ref_dev, ref64, what, axes):
    """bit comparison on the device; on a mismatch the CPU comparer names the coordinates"""
    if not torch.equal(got, ref_dev):
        X.assert_exact(got.cpu(), ref64, what, axes)
        raise AssertionError(f'{what}: differs from the reference only in the sign of a zero')


# ------------------------------------------------------------------------------------------ the fused launch
class Fused:
    """the device side of one fused case: operands uploaded once, launched in several forms"""

    def __init__(self, dz, y, x, w, coef, dx0=None):
        self.M, self.K = dz.shape
        M, K = self.M, self.K
        self.dz_host = dz
        self.y, self.x = Rows(y, off=8, tail=24), Rows(x, off=16, tail=8)
        self.coef = [Vec(a) for a in coef]                                   # scale, shift, mean, invstd, c1, c2
        self.wpd = pack_dgrad(w)
        self.dx0 = None if dx0 is None else t64(dx0).to(BF16).to(DEV)
        self.dz = {}
        self.g = F.geometry(K, M)
        nbytes = ops.fused_1x1_ws_bytes(M, K, K)
        assert nbytes == self.g['grid'] * K * K * 4, (nbytes, self.g)
        assert ops.fused_1x1_stat_slabs(M, K, K, BF16) == self.g['slabs']
        assert ops.fused_1x1_ok(K, K, BF16)
        self.ws_floats = nbytes // 4

    def split(self, Ka):
        if Ka not in self.dz:
            self.dz.clear()
            dz = self.dz_host
            self.dz[Ka] = (Rows(dz, off=16, tail=0), None) if Ka is None else \
                (Rows(np.ascontiguousarray(dz[:, :Ka]), off=16, tail=0), Rows(np.ascontiguousarray(dz[:, Ka:]), off=8, tail=16))
        return self.dz[Ka]

    def run(self, Ka=None, split=None, acc=False, dgrad=True, stats=None):
        """-> (dx Rows or None, Grads or None); split None: no weight gradient"""
        M, K = self.M, self.K
        dza, dzb = self.split(Ka)
        dx = None
        if dgrad:
            dx = Rows(None, K=K, M=M, off=24, tail=16)
            if acc:
                dx.v.copy_(self.dx0.view(1, 1, M, K))
        gr = Grads(K, K, split) if split else None
        ws = Guarded(self.ws_floats)
        rec = ops.rec_conv1x1_bwd_fused(dza.v, dzb.v if dzb else None, self.y.v, *(v.v for v in self.coef), self.x.v, self.wpd if dgrad else None,
                                        dx.v if dgrad else None, gr.a if gr else None, gr.b if gr else None, ws.v, accumulate_dx=acc, stats=stats)
        log = launch([rec])
        name = f'conv1x1_bwd_{K}'
        assert log and log[0] == name and sum(n.startswith('conv1x1_bwd') for n in log) == 1, log
        ws.intact('the weight-gradient workspace')
        for t in [dza, self.y, self.x] + self.coef + ([dzb] if dzb else []) + ([dx] if dx else []) + ([gr] if gr else []):
            t.intact()
        return dx, gr


def exact_coef(c):
    return (c.scale, c.shift, c.mean, c.invstd, c.c1, c.c2)


# ------------------------------------------------------------------------------------------ probe
@functools.lru_cache(maxsize=None)
def probe():
    """(dx equals dz bit for bit, the identity copy is intact)"""
    c = F.fused_case(64, 130, w='identity')
    rng = np.random.RandomState(5)
    dz = F.to_bf16(rng.uniform(-1, 1, (c.M, c.K)))
    dz[dz == 0] = 0.5                                                        # a zero could come back with the other sign
    ones, zeros = np.ones(c.K), np.zeros(c.K)
    d = Fused(dz, c.y, c.x, c.w, (ones, U_SHIFT(c), c.mean, c.invstd, zeros, zeros))
    dx, _ = d.run(split=(c.K, 0))
    got = dx.host()
    same = bool(torch.equal(dx.flat().view(torch.int16), t64(dz).to(BF16).to(DEV).view(torch.int16)))
    close = bool(np.isfinite(got).all() and (np.abs(got - dz) <= 2.0 ** -6 * np.abs(dz)).all())
    return same, close


def U_SHIFT(c):
    return F.U_MIN + np.abs(c.y).max(0)


def test_probe_reciprocal_of_one_is_one():
    same, close = probe()
    assert close, 'the identity filter does not copy dy to dx: the exact legs cannot say anything about v_rcp_f32'
    print(f'F1FIG probe | v_rcp_f32(1.0f) == 1.0f | {int(same)}')
    assert same, "dx differs from dz in its last bits: v_rcp_f32(1.0f) is not 1.0f on this device, silu'(u >= 24) is not exactly 1"


def need_exact():
    same, close = probe()
    if close and not same:
        pytest.skip('v_rcp_f32(1.0f) != 1.0f on this device (test_probe_reciprocal_of_one_is_one): the integer recipe is not exact')


# ------------------------------------------------------------------------------------------ exact legs
@pytest.mark.parametrize('K,name', F.EXACT, ids=[f'{K}-{n}' for K, n in F.EXACT])
def test_fused_backward_is_exact_on_integer_operands(K, name):
    """written dx + dW, accumulated dx, dgrad only and wgrad only; dz cut at Ka, dW cut at (K_a, K_b)"""
    need_exact()
    M = F.row_cases(K)[name]
    c = F.fused_case(K, M)
    d = Fused(c.dz, c.y, c.x, c.w, exact_coef(c), c.dx0)
    ref = {k: t64(getattr(c, k)) for k in ('dx', 'dx_acc', 'dw')}
    dev = {'dx': X.lossless(ref['dx'], BF16).to(DEV), 'dx_acc': X.lossless(ref['dx_acc'], BF16).to(DEV), 'dw': X.lossless(ref['dw'], torch.float32).to(DEV)}
    three = name == 'three-tiles'
    for Ka in ([K - 8] if three else [None, 8, K // 2, K - 8]):
        for split in ([(8, K - 8)] if three else [(K, 0), (8, K - 8), (K // 2, K // 2)]):
            tag = f'K {K} M {M} Ka {Ka} grads {split}'
            dx, gr = d.run(Ka, split)
            equal_or_explain(dx.flat(), dev['dx'], ref['dx'], tag + ' dx', F.AXES_ROWS)
            equal_or_explain(gr.v[:, :, 0, 0], dev['dw'], ref['dw'], tag + ' dW', F.AXES_DW)
            dxa, gra = d.run(Ka, split, acc=True)
            equal_or_explain(dxa.flat(), dev['dx_acc'], ref['dx_acc'], tag + ' dx accumulated', F.AXES_ROWS)
            equal_or_explain(gra.v[:, :, 0, 0], dev['dw'], ref['dw'], tag + ' dW beside the accumulated dx', F.AXES_DW)
            dxo, none = d.run(Ka, None)
            assert none is None and torch.equal(dxo.flat().view(torch.int16), dx.flat().view(torch.int16)), tag + ': dgrad alone gives other bits'
            none, gro = d.run(Ka, split, dgrad=False)
            assert none is None and torch.equal(gro.v.view(torch.int32), gr.v.view(torch.int32)), tag + ': wgrad alone gives other bits'


def make_requests(stat, ranges, nslabs, act, coeffs=None):
    """-> (requests, [(range, y Rows, Guarded slabs, scale Vec, shift Vec)]); stat: {(c0, c1): (y_r, ...)}"""
    reqs, keep = [], []
    for i, r in enumerate(ranges):
        w = r[1] - r[0]
        y = stat[r][0]
        nhw = stat.get('nhw')
        yr = Rows(y, off=8 + 8 * i, tail=16, nhw=nhw)
        sc, sh = (Vec(a) for a in (coeffs[r] if coeffs else (np.ones(w), np.zeros(w))))
        slabs = Guarded(nslabs, 2, w)
        reqs.append(ops.StatRequest(yr.v, sc.v, sh.v, slabs.v, r[0], act))
        keep.append((r, yr, slabs, sc, sh))
    return reqs, keep


def check_exact_slabs(keep, stat, empty_slabs, tag):
    for r, yr, slabs, sc, sh in keep:
        slabs.intact(f'{tag} slabs of {r}')
        _, s1, s2 = stat[r]
        F.assert_slabs_exact(slabs.v, s1, s2, empty_slabs, f'{tag} request {r}')
        yr.intact(), sc.intact(), sh.intact()


STAT_CASES = [(K, n, s) for K in F.STAT_K for n in F.STAT_ROWS for s in F.request_shapes(K)]


@pytest.mark.parametrize('K,name,shape', STAT_CASES, ids=['-'.join(map(str, c)) for c in STAT_CASES])
def test_fused_statistics_are_exact_integer_sums(K, name, shape):
    """act none: both slab rows are integer sums of the FINAL dx; dx and dW bit-equal to the launch without requests"""
    need_exact()
    assert ops.fused_1x1_stat_slabs(1000, 128, 128, BF16) == 0 and ops.fused_1x1_stat_slabs(1000, 96, 96, BF16) == 0
    M = F.row_cases(K)[name]
    c = F.fused_case(K, M, requests=F.all_requests(K))
    ranges = F.request_shapes(K)[shape]
    d = Fused(c.dz, c.y, c.x, c.w, exact_coef(c), c.dx0)
    nslabs = ops.fused_1x1_stat_slabs(M, K, K, BF16)
    assert nslabs == d.g['grid'] > 0
    for acc in (False, True):
        tag = f'K {K} M {M} {shape} acc {acc}'
        plain_dx, plain_gr = d.run(None, (K, 0), acc=acc)
        reqs, keep = make_requests(c.stats[acc], ranges, nslabs, ops.ACT_NONE)
        dx, gr = d.run(None, (K, 0), acc=acc, stats=reqs)
        assert torch.equal(dx.flat().view(torch.int16), plain_dx.flat().view(torch.int16)), tag + ': dx differs from the launch without requests'
        assert torch.equal(gr.v.view(torch.int32), plain_gr.v.view(torch.int32)), tag + ': dW differs from the launch without requests'
        X.assert_exact(dx.flat().cpu(), t64(c.dx_acc if acc else c.dx), tag + ' dx', F.AXES_ROWS)
        check_exact_slabs(keep, c.stats[acc], d.g['empty_slabs'], tag)


# ------------------------------------------------------------------------------------------ data gradient with statistics
class Dgrad:
    def __init__(self, case):
        N, H, W, C, K, R, stride, pad = case
        self.case, self.e = case, X.reference(case)
        e = self.e
        self.M = N * H * W
        self.dy = Rows(X.nhwc(e.dy).reshape(-1, K), off=8, tail=8, nhw=(N, e.Ho, e.Wo))
        self.wpd = pack_dgrad(e.w, R, stride, pad)
        self.dx0 = X.nhwc(e.dx_acc).to(BF16).to(DEV)
        self.g = F.igemm_geometry(N, H, W, C, stride)
        self.nslabs = ops.conv_dgrad_stat_slabs(N, H, W, C, K, R, R, stride, pad, BF16)
        assert self.nslabs == self.g['grid'], (self.nslabs, self.g)
        assert ops.conv_dgrad_stat_slabs(N, H, W, 128, K, R, R, stride, pad, BF16) == 0

    def run(self, acc, stats):
        N, H, W, C, K, R, stride, pad = self.case
        dx = Rows(None, K=C, M=self.M, off=24, tail=16, nhw=(N, H, W))
        if acc:
            dx.v.copy_(self.dx0)
        log = launch([ops.rec_conv_dgrad(self.dy.v, self.wpd, dx.v, R, R, stride, pad, accumulate=acc, stats=stats)])
        assert log == [self.g['name']], (log, self.g['name'])
        dx.intact(), self.dy.intact()
        return dx


DGRAD_CASES = [(n, s) for n in F.DGRAD for s in F.request_shapes(64)]


@pytest.mark.parametrize('name,shape', DGRAD_CASES, ids=['-'.join(c) for c in DGRAD_CASES])
def test_data_gradient_statistics_are_exact_integer_sums(name, shape):
    """hdy_conv_dgrad_stats: dx exact against the float64 convolution, every slab written, integer, and their sum the exact column sums"""
    case = F.DGRAD[name]
    N, H, W, C = case[:4]
    c = F.dgrad_stat_case(*case, F.all_requests(C))
    ranges = F.request_shapes(C)[shape]
    d = Dgrad(case)
    if name.startswith('long'):
        assert d.g['tiles'] > d.g['grid'] and d.g['empty'] > 0
    for acc in (False, True):
        tag = f'{name} {case} {shape} acc {acc}'
        stat = dict(c.stats[acc], nhw=(N, H, W))
        reqs, keep = make_requests(stat, ranges, d.nslabs, ops.ACT_NONE)
        dx = d.run(acc, reqs)
        X.assert_exact(dx.flat().cpu(), t64(c.dx_acc if acc else c.dx), tag + ' dx', F.AXES_ROWS)
        check_exact_slabs(keep, c.stats[acc], d.g['empty_slabs'], tag)


# ------------------------------------------------------------------------------------------ real-valued element-wise phase
REAL = [(K, n, half) for K in F.FUSED_K for n in F.REAL_ROWS for half in (False, True)]


@pytest.mark.parametrize('K,name,half', REAL, ids=[f'{K}-{n}-{"Ka" if h else "one"}' for K, n, h in REAL])
def test_elementwise_phase_through_an_identity_filter(K, name, half):
    """W = identity: dx is the kernel's bf16 dy, compared per element with the float64 restatement (the criterion of the apply pass)"""
    M = F.row_cases(K)[name]
    inputs = bc.bwd_inputs('bf16', K, M)
    dz, y = inputs[:2]
    c1, c2 = F.real_coeffs(inputs)
    ref = F.dy_reference(*inputs, c1, c2)
    x = F.fused_case(K, M).x
    d = Fused(dz, y, x, np.eye(K), tuple(inputs[2:]) + (c1, c2))
    dx, gr = d.run(K // 2 if half else None, (K, 0))
    worst = bn_ref.check_elementwise(dx.host(), ref, True, f'K {K} M {M} Ka {K // 2 if half else None}')
    assert torch.isfinite(gr.v).all()
    figure('elementwise', f'{K}-{M}-{"Ka" if half else "one"}', worst)


# ------------------------------------------------------------------------------------------ real-valued statistics with SiLU
def silu_units(ranges, M, seed):
    """per range: real-valued y_r (bf16 values), scale / shift of bn_cases.coeffs, mean / invstd for the finalize"""
    stat, coeffs, fin = {}, {}, {}
    for i, r in enumerate(ranges):
        w = r[1] - r[0]
        rng = np.random.RandomState(seed + 17 * i)
        stat[r] = (F.to_bf16(rng.standard_normal((M, w)) * 1.2 + 0.3),)
        coeffs[r] = bc.coeffs(w, seed=2)
        fin[r] = (np.full(w, 0.3, np.float32) + rng.uniform(-.01, .01, w).astype(np.float32), rng.uniform(0.7, 0.9, w).astype(np.float32))
    return stat, coeffs, fin


def check_silu_statistics(keep, stat, coeffs, fin, dx_host, n, M, tag):
    worst_sum, worst_fin = 0.0, 0.0
    for r, yr, slabs, sc, sh in keep:
        slabs.intact(tag)
        s = slabs.v.cpu().numpy()
        assert np.isfinite(s).all(), f'{tag} {r}: a slab was never written'
        scale, shift = coeffs[r]
        d = dx_host[:, r[0]:r[1]]
        (s1, s2), (a1, a2) = F.stat_sums_reference(d, stat[r][0], scale, shift, F.ACT_SILU)
        c = F.yardstick(d, stat[r][0], scale, shift, F.ACT_SILU)
        print(f'F1FIG yardstick c | {tag} {r} | {c:.1f}')
        tot = s.astype(np.float64).sum(0)
        worst_sum = max(worst_sum, bn_ref.check_vector(tot[0], s1, bn_ref.sum_bound(a1, n, c), f'{tag} {r} SUM du'),
                        bn_ref.check_vector(tot[1], s2, bn_ref.sum_bound(a2, n, c), f'{tag} {r} SUM du y'))
        mean, invstd = fin[r]
        w = r[1] - r[0]
        dbeta, dgamma, c1, c2, bb, bg = bn_ref.slab_finalize(s, M, mean, invstd)
        mu, inv, dg, db, k1, k2 = Vec(mean), Vec(invstd), Vec(K=w), Vec(K=w), Vec(K=w), Vec(K=w)
        launch([ops.rec_bn_bwd_finalize_slabs(slabs.v, M, mu.v, inv.v, dg.v, db.v, k1.v, k2.v)])
        worst_fin = max(worst_fin, bn_ref.check_vector(db.host(), dbeta, bb, f'{tag} {r} dbeta'), bn_ref.check_vector(dg.host(), dgamma, bg, f'{tag} {r} dgamma'),
                        bn_ref.check_vector(k1.host(), c1, bb / M, f'{tag} {r} c1'), bn_ref.check_vector(k2.host(), c2, bg / M, f'{tag} {r} c2'))
        for v in (mu, inv, dg, db, k1, k2):
            v.intact()
    return worst_sum, worst_fin


def test_fused_statistics_with_silu():
    """fused 64 at two tiles per workgroup: du from the dx bits read back and the float64 silu'"""
    K, M = 64, F.row_cases(64)['two-tiles']
    c = F.fused_case(K, M)
    d = Fused(c.dz, c.y, c.x, c.w, exact_coef(c), c.dx0)
    ranges = F.request_shapes(K)['split8']
    stat, coeffs, fin = silu_units(ranges, M, 11)
    reqs, keep = make_requests(stat, ranges, d.g['grid'], ops.ACT_SILU, coeffs)
    dx, _ = d.run(None, (K, 0), acc=True, stats=reqs)
    ws, wf = check_silu_statistics(keep, stat, coeffs, fin, dx.host(), F.chain('fused', K, d.g['tpb']), M, 'fused 64')
    figure('silu statistics', 'fused-64-two-tiles sums', ws)
    figure('silu statistics', 'fused-64-two-tiles finalize', wf)


@pytest.mark.parametrize('name', ['3x3', 's2-walk'])
def test_data_gradient_statistics_with_silu(name):
    case = F.DGRAD[name]
    N, H, W, C = case[:4]
    d = Dgrad(case)
    ranges = F.request_shapes(C)['split8']
    stat, coeffs, fin = silu_units(ranges, d.M, 23)
    reqs, keep = make_requests(dict(stat, nhw=(N, H, W)), ranges, d.nslabs, ops.ACT_SILU, coeffs)
    dx = d.run(True, reqs)
    ws, wf = check_silu_statistics(keep, stat, coeffs, fin, dx.host(), F.chain('igemm', C, d.g['tpb']), d.M, name)
    figure('silu statistics', f'{d.g["name"]} sums', ws)
    figure('silu statistics', f'{d.g["name"]} finalize', wf)
