"""csrc/bn_act.hip driven directly (the ops.rec_* wrappers, no model) on an MI355X against the float64 restatement tests/bn_ref.py, on the
cases of tests/bn_cases.py (tests/test_bn_ref_host.py proves on the CPU what each contains: 1 to 2100 statistic slabs with and without the
two-stage workspace, clamped load slots, channel slices and pairs, a second column chunk of 1 and of 12 vectors with dead lanes, row
blocks with every per-lane row count mod 4, empty row blocks, 1024 row blocks, NaN and infinities, exact zeros, |u| up to 100).

Every tensor lives in a pitched buffer at a nonzero channel offset with 7.0 outside; every output buffer is prefilled with 7.0, inside
too.  After each call the 7.0 outside must be intact; inside, the comparison with the reference shows that the prefill is gone.

Criteria (derivations in bn_ref): finalize outputs per channel within 1 to 3 fp32 ulps of the largest term; fp32 z / dy within
1e-4 |ref| + 0.2e-4 rms(ref) for every element, bf16 z / dy within 2^-8 |ref| on top; per-channel sums within
(n + c) 2^-24 SUM |term|, n the longest fp32 chain of the launch geometry, c the yardstick (bn_ref.yardstick_c: four times what a plain
float32 evaluation of the same formulas loses per term, plus the final cast; 1 where the terms are exact).  Kernel against kernel: equal
bits.  No bound comes from a kernel's output and no element is excluded.

Measured on an MI355X, worst case of each group, error in units of its bound (must stay <= 1):

    group (cases)                            worst error / bound (case)            median
    finalize (20)                            0.559 (twostage-2100)                 0.458
    forward (24 x 3 activations x residual)  0.970 (bf16-2056-257)                 0.693    fp32 alone: 0.007 at most
    forward, |u| to 100 / zeros / nonfinite  0.965 / 0.970 / 0.968 (bf16)          0.96     fp32 alone: 0.001 / 0.004 / 0.006
    forward pair (6)                         0.968 (bf16-2144-2048)                0.949
    backward sums (82)                       0.721 (bf16-2056-1-silu)              0.040
    backward dy (82)                         0.970 (bf16-48-32769-silu)            0.848
    backward pair sums (12)                  0.071 (f32-48-65-16-none)             0.057
    backward pair dy (12)                    0.967 (bf16-2144-65-2048-silu)        0.954
    backward finalize of slabs (4)           0.882 (1023)                          0.849
    colsum (18)                              0.756 (bf16-1072-1, accumulated)      0.024
    SyncBatchNorm                            0.395 (bwd_coeffs_sums); the fp64 slab sums: 0.000 of 1e-12
    eval table                               0.322

A bf16 output sits at 0.97 by construction: half a bf16 ulp is 2^-8 / (2^-8 + 1e-4) of its bound and some element always rounds that far.

Measured c: 3.8 to 13.0 for every case with 34 rows or more (act none 3.8-6.6, SiLU 5.5-13.0), 141 to 522 for SiLU at M = 1, where a sum
is one term next to the zero of silu' (test_bn_ref_host.test_yardstick_c_is_a_few_roundings).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bn_cases as bc  # noqa: E402
import bn_ref  # noqa: E402
from hd_yolo_amd import _lib, ops  # noqa: E402

DEV = torch.device('cuda', 0)
OFF, TAIL, PAD = 8, 8, 4                      # channel offset and trailing channels of a tensor's buffer; floats around a parameter vector
INT_VIEW = {torch.float32: torch.int32, torch.bfloat16: torch.int16}
ACT_NAME = {0: 'none', 1: 'silu', 2: 'relu'}


def bits(t):
    return t.contiguous().view(INT_VIEW[t.dtype])


def figure(group, what, worst):
    print(f'BNFIG {group} | {what} | {worst:.3f}')
    return worst


# ------------------------------------------------------------------------------------------ buffers
class Rows:
    """an [M, K] tensor as the NHWC view [1, 1, M, K] at channel OFF of a pitch K + OFF + TAIL buffer, 7.0 everywhere else (a=None: the
    view is 7.0 too, an output's prefill)"""

    def __init__(self, a, dt, K=None, M=None, off=OFF, tail=TAIL):
        M, K = a.shape if a is not None else (M, K)
        self.K, self.off = K, off
        self.buf = torch.full((1, 1, M, K + off + tail), bc.POISON, dtype=bc.TORCH[dt], device=DEV)
        self.v = self.buf[..., off:off + K]
        if a is not None:
            self.v.copy_((torch.from_numpy(a) if isinstance(a, np.ndarray) else a).to(bc.TORCH[dt]).view(1, 1, M, K))

    def host(self):
        return self.v.float().cpu().numpy().reshape(-1, self.K).astype(np.float64)

    def intact(self):
        assert (self.buf[..., :self.off] == bc.POISON).all() and (self.buf[..., self.off + self.K:] == bc.POISON).all(), 'poison outside the view overwritten'


class Vec:
    """a per-channel fp32 vector in the middle of a 7.0-filled buffer (a=None: prefilled output of K floats)"""

    def __init__(self, a=None, K=None, dtype=torch.float32):
        K = len(a) if a is not None else K
        self.K = K
        self.buf = torch.full((K + 2 * PAD,), bc.POISON, dtype=dtype, device=DEV)
        self.v = self.buf[PAD:PAD + K]
        if a is not None:
            self.v.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(dtype))

    def host(self):
        return self.v.cpu().numpy().astype(np.float64)

    def intact(self):
        assert (self.buf[:PAD] == bc.POISON).all() and (self.buf[PAD + self.K:] == bc.POISON).all(), 'poison around a vector overwritten'


def launch(records):
    """run the records; returns the kernel families the library chose"""
    _lib.dispatch_log(reset=True)
    ops.run(records)
    torch.cuda.synchronize()
    return _lib.dispatch_log(reset=True)


# ------------------------------------------------------------------------------------------ finalize
@pytest.mark.parametrize('name', list(bc.FINALIZE))
def test_finalize_matches_the_float64_restatement(name):
    c = bc.finalize_inputs(name)
    K, k0, mt, Ka = c['K'], c['k0'], c['mtiles'], c['Ka']
    stats = torch.from_numpy(c['slabs']).to(DEV)
    par = {k: Vec(c[k]) for k in ('gamma', 'beta', 'rm', 'rv')}
    out = [Vec(K=K) for _ in range(4)]
    ws = None
    if c['ws']:
        nbytes = _lib.query('hdy_bn_finalize_workspace_bytes', mt, K)
        assert nbytes == 32 * 2 * K * 8
        wsbuf = torch.full((nbytes // 8 + 2,), bc.POISON, dtype=torch.float64, device=DEV)
        ws = wsbuf[:nbytes // 8]
    o = [v.v for v in out]
    if Ka:
        bn_a = tuple(par[k].v[:Ka] for k in ('gamma', 'beta', 'rm', 'rv'))
        bn_b = (par['gamma'].v[Ka:], par['beta'].v[Ka:], None, None)                     # the second module keeps no running statistics
        rec = ops.rec_bn_finalize_pair(stats, mt, K, Ka, c['count'], bn_a, bn_b, *o, ws=ws)
    else:
        rec = ops.rec_bn_finalize(stats[:, :, k0:], mt, K, c['count'], par['gamma'].v, par['beta'].v, par['rm'].v, par['rv'].v, *o,
                                  stats_ld=c['stats_ld'], ws=ws)
    log = launch([rec])
    assert log == ['bn_finalize_2stage' if c['ws'] else 'bn_finalize'], log
    view = bc.finalize_view(c)
    args = (view, c['count'], c['gamma'], c['beta'], c['rm'], c['rv'], bc.EPS, bc.MOMENTUM)
    ref, bounds = list(bn_ref.finalize(*args)), bn_ref.finalize_bounds(*args)
    got = [v.host() for v in out] + [par['rm'].host(), par['rv'].host()]
    if Ka:                                                                               # [Ka, K): untouched running statistics
        assert np.array_equal(got[4][Ka:], c['rm'][Ka:]) and np.array_equal(got[5][Ka:], c['rv'][Ka:])
        ref[4][Ka:], ref[5][Ka:] = c['rm'][Ka:], c['rv'][Ka:]
    figure('finalize', name, bn_ref.check_finalize(got, ref, bounds, name))
    for v in list(par.values()) + out:
        v.intact()
    assert torch.equal(stats.cpu(), torch.from_numpy(c['slabs']))
    assert np.array_equal(par['gamma'].host(), c['gamma']) and np.array_equal(par['beta'].host(), c['beta'])
    if ws is not None:
        assert (wsbuf[nbytes // 8:] == bc.POISON).all()


# ------------------------------------------------------------------------------------------ forward
def forward_case(dt, K, M, kind, acts, with_res, group):
    y, res, scale, shift = bc.fwd_inputs(dt, K, M, kind)
    yd, rd, sc, sh = Rows(y, dt), Rows(res, dt, off=16, tail=0), Vec(scale), Vec(shift)
    worst = 0.0
    for act in acts:
        for r in with_res:
            z = Rows(None, dt, K=K, M=M, off=24)
            launch([ops.rec_bn_act_fwd(yd.v, sc.v, sh.v, z.v, res=rd.v if r else None, act=act)])
            ref = bn_ref.forward(y, scale, shift, act, res if r else None)
            worst = max(worst, bn_ref.check_elementwise(z.host(), ref, dt == 'bf16', f'{dt} K {K} M {M} {kind} act {ACT_NAME[act]} res {r}'))
            for t in (yd, rd, sc, sh, z):
                t.intact()
    assert np.array_equal(yd.host(), y, equal_nan=True) and np.array_equal(rd.host(), res)
    return figure(group, f'{dt}-{K}-{M}-{kind}', worst)


@pytest.mark.parametrize('case', bc.FWD, ids=bc.case_id)
def test_forward_matches_the_float64_restatement(case):
    """three activations, with and without the residual"""
    forward_case(*case, 'plain', bc.ACTS, (False, True), 'forward')


@pytest.mark.parametrize('act', bc.ACTS, ids=[ACT_NAME[a] for a in bc.ACTS])
@pytest.mark.parametrize('kind', bc.SPECIAL)
@pytest.mark.parametrize('dt', bc.DTYPES)
def test_forward_on_wide_zero_and_nonfinite_pre_activations(dt, kind, act):
    """|u| up to 100, u exactly 0, and NaN / +Inf / -Inf planted in y: the output is NaN exactly where the reference's is (a ReLU written
    as fmaxf(u, 0) returns 0 for a NaN) and carries the reference's infinities"""
    forward_case(dt, bc.FWD_K[dt][3], bc.SPECIAL_M, kind, (act,), (False, True), 'forward ' + kind)


@pytest.mark.parametrize('dt,K,Ka', [(dt, K, Ka) for dt in bc.DTYPES for K, Ka in bc.PAIRS[dt]])
def test_forward_pair_writes_both_destinations(dt, K, Ka):
    """channels [0, Ka) to one buffer, the rest to another of a different pitch; the pair form has no residual"""
    M = 35
    y, _, scale, shift = bc.fwd_inputs(dt, K, M)
    yd, sc, sh = Rows(y, dt), Vec(scale), Vec(shift)
    worst = 0.0
    for act in bc.ACTS:
        za, zb = Rows(None, dt, K=Ka, M=M, off=16), Rows(None, dt, K=K - Ka, M=M, off=8, tail=16)
        launch([ops.rec_bn_act_fwd_pair(yd.v, sc.v, sh.v, za.v, zb.v, act=act)])
        ref = bn_ref.forward(y, scale, shift, act)
        got = np.concatenate([za.host(), zb.host()], 1)
        worst = max(worst, bn_ref.check_elementwise(got, ref, dt == 'bf16', f'pair {dt} {K} {Ka} act {ACT_NAME[act]}'))
        one = Rows(None, dt, K=K, M=M)                                                   # and bit-equal to the single-destination call
        launch([ops.rec_bn_act_fwd(yd.v, sc.v, sh.v, one.v, act=act)])
        assert torch.equal(bits(torch.cat([za.v, zb.v], 3)), bits(one.v))
        for t in (yd, za, zb, sc, sh):
            t.intact()
    figure('forward pair', f'{dt}-{K}-{Ka}', worst)


# ------------------------------------------------------------------------------------------ backward
class Backward:
    """the device side of one backward case: uploaded once, run in several forms"""

    def __init__(self, dt, K, M, Ka=None):
        self.dt, self.K, self.M, self.Ka = dt, K, M, Ka
        self.inputs = bc.bwd_inputs(dt, K, M)
        dz, y = self.inputs[:2]
        self.y = Rows(y, dt)
        if Ka:
            self.dza, self.dzb = Rows(dz[:, :Ka].copy(), dt, off=16), Rows(dz[:, Ka:].copy(), dt, off=8, tail=16)
        else:
            self.dz = Rows(dz, dt, off=16, tail=0)
        self.coef = [Vec(a) for a in self.inputs[2:]]
        self.ws = torch.full((ops.bn_bwd_ws_floats(M, K) + 8,), bc.POISON, device=DEV)
        assert ops.bn_bwd_blocks(M) == bc.bn_bwd_blocks(M)

    def run(self, act, dy=True, accumulate=False, frozen=False, old=None):
        """-> (dy, dgamma, dbeta, c1, c2, dispatch log); old: what the gradient buffers hold before the call"""
        K, M, Ka = self.K, self.M, self.Ka
        self.ws.fill_(bc.POISON)
        out = Rows(None, self.dt, K=K, M=M, off=24) if dy else None
        dg, db = Vec(old[0] if old else None, K=K), Vec(old[1] if old else None, K=K)
        sc, sh, mu, inv = (v.v for v in self.coef)
        stats = (None, None) if frozen else (mu, inv)
        if Ka:
            rec = ops.rec_bn_act_bwd_pair(self.dza.v, self.dzb.v, self.y.v, sc, sh, *stats, out.v if dy else None, dg.v[:Ka], db.v[:Ka], dg.v[Ka:], db.v[Ka:],
                                          self.ws, accumulate=accumulate, act=act)
        else:
            rec = ops.rec_bn_act_bwd(self.dz.v, self.y.v, sc, sh, *stats, out.v if dy else None, dg.v, db.v, self.ws, accumulate=accumulate, act=act)
        log = launch([rec])
        c1, c2 = (t.cpu().numpy().astype(np.float64) for t in ops.bn_bwd_coeffs(self.ws, M, K))
        for t in [self.y, dg, db] + self.coef + ([out] if dy else []) + ([self.dza, self.dzb] if Ka else [self.dz]):
            t.intact()
        assert (self.ws[-8:] == bc.POISON).all()
        self.out = out
        return (out.host() if dy else None), dg.host(), db.host(), c1, c2, log

    def apply(self, act, c1, c2):
        """dy from given c1 / c2 through the apply pass alone"""
        out = Rows(None, self.dt, K=self.K, M=self.M, off=24)
        k1, k2 = Vec(c1.astype(np.float32)), Vec(c2.astype(np.float32))
        sc, sh, mu, inv = (v.v for v in self.coef)
        dza, dzb = (self.dza.v, self.dzb.v) if self.Ka else (self.dz.v, None)
        launch([ops.rec_bn_act_bwd_apply(dza, dzb, self.y.v, sc, sh, mu, inv, k1.v, k2.v, out.v, act=act)])
        out.intact()
        return out


def check_backward(d, act, group):
    dt, K, M = d.dt, d.K, d.M
    ref = bn_ref.backward(*d.inputs, act, M)
    a1, a2 = bn_ref.backward_abs_sums(*d.inputs, act)
    c = bn_ref.yardstick_c(*d.inputs, act)
    tag = f'{dt}-{K}-{M}' + (f'-{d.Ka}' if d.Ka else '') + f'-{ACT_NAME[act]}'
    finalize_name = 'bn_bwd_finalize_wide' if bc.bn_bwd_blocks(M) >= 1024 else 'bn_bwd_finalize'
    worst_sum, worst_dy = 0.0, 0.0
    for eight in ((False, True) if dt == 'bf16' else (False,)):                          # bf16: the four-channel kernel, then the eight-channel one
        with _lib.option('HDY_NO_BN_REDUCE4', int(eight)):
            dy, dg, db, c1, c2, log = d.run(act)
        reduce4 = dt == 'bf16' and not eight
        assert log == ['bn_bwd_reduce4' if reduce4 else 'bn_bwd_reduce', finalize_name], log
        n = bc.chain(M, K, 4 if reduce4 else bc.VE[dt])
        b1, b2 = bn_ref.sum_bound(a1, n, c), bn_ref.sum_bound(a2, n, c)
        what = f'{tag} {log[0]}'
        worst_sum = max(worst_sum, bn_ref.check_vector(db, ref[1], b1, what + ' dbeta'), bn_ref.check_vector(dg, ref[2], b2, what + ' dgamma'),
                        bn_ref.check_vector(c1, ref[3], b1 / M, what + ' c1'), bn_ref.check_vector(c2, ref[4], b2 / M, what + ' c2'))
        worst_dy = max(worst_dy, bn_ref.check_elementwise(dy, ref[5], dt == 'bf16', what + ' dy'))
        assert torch.equal(bits(d.apply(act, c1, c2).v), bits(d.out.v)), what + ': the apply pass alone gives other bits from the same c1 / c2'
    # accumulate into gradients already there, statistics only (dy = None)
    old = (np.linspace(-2, 2, K).astype(np.float32), np.linspace(3, -1, K).astype(np.float32))
    none, dg, db, c1, c2, log = d.run(act, dy=False, accumulate=True, old=old)
    n = bc.chain(M, K, 4)                                                                # fp32 and the four-channel kernel: 4 elements per lane
    b1, b2 = bn_ref.sum_bound(a1, n, c), bn_ref.sum_bound(a2, n, c)
    assert none is None and log[0] == ('bn_bwd_reduce4' if dt == 'bf16' else 'bn_bwd_reduce')
    extra = [bn_ref.U32 * (np.abs(o) + np.abs(r)) for o, r in zip(old, (ref[2], ref[1]))]
    worst_sum = max(worst_sum, bn_ref.check_vector(dg, old[0] + ref[2], bn_ref.sum_bound(a2, n, c, extra[0]), tag + ' dgamma accumulated'),
                    bn_ref.check_vector(db, old[1] + ref[1], bn_ref.sum_bound(a1, n, c, extra[1]), tag + ' dbeta accumulated'),
                    bn_ref.check_vector(c1, ref[3], b1 / M, tag + ' c1, statistics only'), bn_ref.check_vector(c2, ref[4], b2 / M, tag + ' c2, statistics only'))
    # frozen BatchNorm: the apply pass alone, no parameter gradients
    dy, dg, db, _, _, log = d.run(act, frozen=True)
    assert log == [] and (dg == bc.POISON).all() and (db == bc.POISON).all()
    worst_dy = max(worst_dy, bn_ref.check_elementwise(dy, bn_ref.backward_frozen(*d.inputs[:4], act), dt == 'bf16', tag + ' frozen dy'))
    figure(group + ' sums', tag, worst_sum)
    figure(group + ' dy', tag, worst_dy)


@pytest.mark.parametrize('act', bc.BWD_ACTS, ids=[ACT_NAME[a] for a in bc.BWD_ACTS])
@pytest.mark.parametrize('case', bc.BWD, ids=bc.case_id)
def test_backward_matches_the_float64_restatement(case, act):
    """trained (both reduce kernels in bf16), accumulated with dy = None, and frozen"""
    check_backward(Backward(*case), act, 'backward')


@pytest.mark.parametrize('act', bc.BWD_ACTS, ids=[ACT_NAME[a] for a in bc.BWD_ACTS])
@pytest.mark.parametrize('case', bc.BWD_PAIRS, ids=bc.case_id)
def test_backward_pair_matches_the_float64_restatement(case, act):
    """two gradient sources of different pitches, parameter gradients split at Ka"""
    dt, K, Ka, M = case
    check_backward(Backward(dt, K, M, Ka=Ka), act, 'backward pair')


@pytest.mark.parametrize('nslabs', bc.SLAB_COUNTS)
def test_backward_finalize_of_producer_slabs(nslabs):
    """rec_bn_bwd_finalize_slabs: (SUM du, SUM du * y) slabs of another kernel's epilogue, 1023 (8 x 32 lanes) to 2049 slabs (8 x 128)"""
    slabs, count, mean, invstd = bc.slab_inputs(nslabs)
    K = bc.SLAB_K
    dbeta, dgamma, c1, c2, bb, bg = bn_ref.slab_finalize(slabs, count, mean, invstd)
    sd = torch.from_numpy(slabs).to(DEV)
    worst = 0.0
    for acc in (False, True):
        old = np.linspace(-2, 2, K).astype(np.float32)
        mu, inv, dg, db, k1, k2 = Vec(mean), Vec(invstd), Vec(old if acc else None, K=K), Vec(old if acc else None, K=K), Vec(K=K), Vec(K=K)
        log = launch([ops.rec_bn_bwd_finalize_slabs(sd, count, mu.v, inv.v, dg.v, db.v, k1.v, k2.v, accumulate=acc)])
        assert log == ['bn_bwd_finalize_wide' if nslabs >= 1024 else 'bn_bwd_finalize'], log
        base = old.astype(np.float64) if acc else 0.0
        ex_b, ex_g = (bn_ref.U32 * (np.abs(old) + np.abs(r)) if acc else 0.0 for r in (dbeta, dgamma))
        worst = max(worst, bn_ref.check_vector(db.host(), base + dbeta, bb + ex_b, 'dbeta'), bn_ref.check_vector(dg.host(), base + dgamma, bg + ex_g, 'dgamma'),
                    bn_ref.check_vector(k1.host(), c1, bb / count, 'c1'), bn_ref.check_vector(k2.host(), c2, bg / count, 'c2'))
        for v in (mu, inv, dg, db, k1, k2):
            v.intact()
    assert torch.equal(sd.cpu(), torch.from_numpy(slabs))
    figure('backward finalize of slabs', str(nslabs), worst)


# ------------------------------------------------------------------------------------------ column sums, add
@pytest.mark.parametrize('case', bc.COLSUM, ids=bc.case_id)
def test_colsum_matches_the_float64_sum(case):
    """the detection head's bias gradient: plain column sums (terms exact: c = 1 for the cast), stored and accumulated"""
    dt, K, M = case
    dz = bc.colsum_inputs(dt, K, M)
    ref = dz.double().sum(0).numpy()
    bound = bn_ref.sum_bound(dz.double().abs().sum(0).numpy(), bc.chain(M, K, bc.VE[dt]), 1.0)
    assert ops.bn_bwd_blocks(M) == bc.bn_bwd_blocks(M)
    d = Rows(dz, dt)
    ws = torch.full((ops.bn_bwd_ws_floats(M, K) + 8,), bc.POISON, device=DEV)
    worst = 0.0
    for acc in (False, True):
        old = np.linspace(-2, 2, K).astype(np.float32)
        out = Vec(old if acc else None, K=K)
        log = launch([ops.rec_colsum(d.v, out.v, ws, accumulate=acc)])
        assert log == ['bn_bwd_reduce', 'bn_bwd_finalize'], log
        extra = bn_ref.U32 * (np.abs(old) + np.abs(ref)) if acc else 0.0
        worst = max(worst, bn_ref.check_vector(out.host(), ref + (old if acc else 0.0), bound + extra, f'colsum {case} accumulate {acc}'))
        out.intact(), d.intact()
        assert (ws[-8:] == bc.POISON).all()
    figure('colsum', bc.case_id(case), worst)


@pytest.mark.parametrize('case', bc.ADD, ids=bc.case_id)
def test_add_inplace_is_the_sum_rounded_once(case):
    dt, K, M = case
    y, res, _, _ = bc.fwd_inputs(dt, K, M)
    a, b = Rows(y, dt), Rows(res, dt, off=16, tail=0)
    want = (torch.from_numpy(y) + torch.from_numpy(res)).to(bc.TORCH[dt]).view(1, 1, M, K)          # fp32 sum of the operands, rounded once
    launch([ops.rec_add_inplace(a.v, b.v)])
    assert torch.equal(bits(a.v.cpu()), bits(want))
    a.intact(), b.intact()
    assert np.array_equal(b.host(), res)


# ------------------------------------------------------------------------------------------ SyncBatchNorm, eval table
def test_sync_batchnorm_on_two_emulated_ranks():
    """two slab sets -> rec_bn_slab_sums each, the 2K + 1 doubles added on the device, rec_bn_finalize_sums on a channel slice with a pair
    split: equal to the finalize of the concatenated slabs with the summed count; rec_bn_bwd_coeffs_sums likewise"""
    sets, counts, par = bc.sync_inputs()
    Ktot, k0, K, Ka = (bc.SYNC[k] for k in ('Ktot', 'k0', 'K', 'Ka'))
    sums = []
    for slabs, count in zip(sets, counts):
        s = Vec(K=2 * Ktot + 1, dtype=torch.float64)
        launch([ops.rec_bn_slab_sums(torch.from_numpy(slabs).to(DEV), len(slabs), Ktot, count, s.v)])
        s.intact()
        ref, mag = bn_ref.sync_sums([slabs], [count]), np.abs(slabs.astype(np.float64)).sum(0).reshape(-1)
        assert s.host()[2 * Ktot] == count
        figure('sync', 'fp64 sums / 1e-12', bn_ref.check_vector(s.host()[:2 * Ktot], ref[:2 * Ktot], 1e-12 * mag, 'slab sums'))
        sums.append(s.v)
    total = (sums[0] + sums[1]).contiguous()
    p = {k: Vec(v) for k, v in par.items()}
    out = [Vec(K=K) for _ in range(4)]
    bn_a = tuple(p[k].v[:Ka] for k in ('gamma', 'beta', 'rm', 'rv'))
    bn_b = tuple(p[k].v[Ka:] for k in ('gamma', 'beta', 'rm', 'rv'))
    launch([ops.rec_bn_finalize_sums(total, Ktot, k0, K, Ka, bn_a, bn_b, *(v.v for v in out))])
    both = np.concatenate(sets)[:, :, k0:k0 + K]
    args = (both, sum(counts), par['gamma'], par['beta'], par['rm'], par['rv'], bc.EPS, bc.MOMENTUM)
    got = [v.host() for v in out] + [p['rm'].host(), p['rv'].host()]
    figure('sync', 'finalize_sums', bn_ref.check_finalize(got, bn_ref.finalize(*args), bn_ref.finalize_bounds(*args), 'finalize_sums'))
    for v in list(p.values()) + out:
        v.intact()
    # backward coefficients from the global [SUM du | SUM du * xhat | count]: the same sums stand in for the ranks' partial slabs
    k1, k2 = Vec(K=Ktot), Vec(K=Ktot)
    launch([ops.rec_bn_bwd_coeffs_sums(total, Ktot, k1.v, k2.v)])
    c1, c2 = bn_ref.sync_coeffs(bn_ref.sync_sums(sets, counts))
    figure('sync', 'bwd_coeffs_sums', max(bn_ref.check_vector(k1.host(), c1, bn_ref.ULP * np.abs(c1), 'c1'),
                                          bn_ref.check_vector(k2.host(), c2, bn_ref.ULP * np.abs(c2), 'c2')))
    k1.intact(), k2.intact()


def test_eval_table_equals_the_single_call_and_sees_a_parameter_change():
    """ops.BnEvalTable over five BatchNorms (K = 1 .. 700: fewer and more channels than a workgroup's 256 lanes) against rec_bn_eval_coeffs,
    bit for bit; skip_unchanged skips while nothing changed and recomputes after an in-place parameter update"""
    table = ops.BnEvalTable(DEV)
    mods = []
    for K in bc.EVAL_K:
        p = {k: torch.from_numpy(v).to(DEV) for k, v in bc.eval_inputs(K).items()}
        p['scale'], p['shift'] = Vec(K=K), Vec(K=K)
        table.add(p['gamma'], p['beta'], p['rm'], p['rv'], p['scale'].v, p['shift'].v)
        mods.append(p)

    def check(what):
        worst = 0.0
        for p in mods:
            one_s, one_h = Vec(K=p['scale'].K), Vec(K=p['scale'].K)
            launch([ops.rec_bn_eval_coeffs(p['gamma'], p['beta'], p['rm'], p['rv'], one_s.v, one_h.v)])
            assert torch.equal(bits(p['scale'].v), bits(one_s.v)) and torch.equal(bits(p['shift'].v), bits(one_h.v)), what
            host = [p[k].cpu().numpy() for k in ('gamma', 'beta', 'rm', 'rv')]
            (rs, rh), (bs, bh) = bn_ref.eval_coeffs(*host, bc.EPS), bn_ref.eval_bounds(*host, bc.EPS)
            worst = max(worst, bn_ref.check_vector(one_s.host(), rs, bs, what + ' scale'), bn_ref.check_vector(one_h.host(), rh, bh, what + ' shift'))
            for v in (p['scale'], p['shift'], one_s, one_h):
                v.intact()
        figure('eval table', what, worst)

    table.run(skip_unchanged=True)
    torch.cuda.synchronize()
    check('first run')
    for p in mods:                                   # through .data: no version bump, so an unchanged table must leave these alone
        p['scale'].v.data.fill_(bc.POISON)
        p['shift'].v.data.fill_(bc.POISON)
    table.run(skip_unchanged=True)
    torch.cuda.synchronize()
    assert all((p['scale'].v == bc.POISON).all() and (p['shift'].v == bc.POISON).all() for p in mods), 'an unchanged table was recomputed'
    for p, K in zip(mods, bc.EVAL_K):                # in-place updates, as an optimizer step or load_state_dict makes them
        new = bc.eval_inputs(K, bump=1)
        p['gamma'].copy_(torch.from_numpy(new['gamma']))
        p['rv'].mul_(1.5)
    table.run(skip_unchanged=True)
    torch.cuda.synchronize()
    check('after a parameter change')
