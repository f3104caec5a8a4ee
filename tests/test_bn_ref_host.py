"""CPU checks of the BatchNorm restatement (tests/bn_ref.py) and of the cases the direct GPU tests run (tests/bn_cases.py).

1. The restatement equals torch float64 autograd (F.batch_norm(training=True), then SiLU / ReLU / identity, plus the residual) at 1e-12 on
   every case torch accepts: forward, dy, dgamma, dbeta, running statistics.  torch refuses one value per channel (count == 1): that case
   is checked against hand values.  The BatchNorm backward exists for no activation and SiLU, as in the kernels.
2. Each case contains what its name claims (chunk widths, dead lanes, empty row blocks, per-lane row counts mod 4, two-stage groups, the
   enlarged last slab): asserted below, so that an edited case that loses its feature fails here.
3. Every comparer rejects a reference perturbed by twice its bound and accepts one perturbed by half of it.
The restatement excludes nothing and there is no skip list.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_cases as bc
import bn_ref

SMALL = [c for c in bc.BWD if c[1] * c[2] <= 300000]
TORCH_ACT = {bn_ref.ACT_NONE: lambda t: t, bn_ref.ACT_SILU: F.silu, bn_ref.ACT_RELU: F.relu}


def close(got, ref, what):
    ref = np.asarray(ref, np.float64)
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-12 * max(float(np.abs(ref).max()), 1e-300), err_msg=what)


# ------------------------------------------------------------------------------------------ 1. the restatement against torch float64
@pytest.mark.parametrize('case', SMALL, ids=bc.case_id)
def test_restatement_equals_torch_float64_autograd(case):
    dt, K, M = case
    dz, y, _, _, _, _ = bc.bwd_inputs(dt, K, M)
    gamma, beta = (a.astype(np.float64) for a in bc.coeffs(K, seed=1))
    res = bc.fwd_inputs(dt, K, M)[1] if (dt, K, M) in bc.FWD else np.flip(dz, 0).copy()
    rm, rv = np.linspace(-0.5, 0.5, K), np.linspace(0.5, 1.5, K)
    y64 = y.astype(np.float64)
    slabs = np.stack([y64.sum(0), (y64 * y64).sum(0)])[None]
    scale, shift, mean, invstd, rm1, rv1 = bn_ref.finalize(slabs, M, gamma, beta, rm, rv, bc.EPS, bc.MOMENTUM)
    if M == 1:
        # hand values: mean = y, biased variance 0 (kept biased for the running value), so u = beta for every element
        close(mean, y64[0], 'mean')
        close(invstd, np.full(K, bc.EPS ** -0.5), 'invstd')
        close(scale, gamma * bc.EPS ** -0.5, 'scale')
        close(rm1, (1 - bc.MOMENTUM) * rm + bc.MOMENTUM * y64[0], 'running_mean')
        close(rv1, (1 - bc.MOMENTUM) * rv, 'running_var')
        b = beta
        np.testing.assert_allclose(bn_ref.forward(y, scale, shift, bn_ref.ACT_RELU, res), np.maximum(b, 0) + res, rtol=0, atol=1e-9)
        np.testing.assert_allclose(bn_ref.forward(y, scale, shift, bn_ref.ACT_SILU), (b / (1 + np.exp(-b)))[None], rtol=0, atol=1e-9)
        du, dbeta, dgamma, c1, c2, dy = bn_ref.backward(dz, y, scale, shift, mean, invstd, bn_ref.ACT_NONE, 1)
        assert np.array_equal(du, dz) and np.array_equal(dbeta, dz[0]) and np.array_equal(c1, dz[0])
        assert not dgamma.any() and not c2.any() and not dy.any()
        return
    for act in bc.ACTS:
        for with_res in (False, True):
            yt = torch.from_numpy(y64).requires_grad_(True)
            g, b = (torch.from_numpy(a.copy()).requires_grad_(True) for a in (gamma, beta))
            rmt, rvt = torch.from_numpy(rm.copy()), torch.from_numpy(rv.copy())
            z = TORCH_ACT[act](F.batch_norm(yt, rmt, rvt, g, b, True, bc.MOMENTUM, bc.EPS))
            if with_res:
                z = z + torch.from_numpy(res.astype(np.float64))
            z.backward(torch.from_numpy(dz.astype(np.float64)))
            what = f'{case} act {act} res {with_res}'
            close(bn_ref.forward(y, scale, shift, act, res if with_res else None), z.detach().numpy(), what + ' z')
            close(rm1, rmt.numpy(), what + ' running_mean')
            close(rv1, rvt.numpy(), what + ' running_var')
            if act in bc.BWD_ACTS:
                du, dbeta, dgamma, c1, c2, dy = bn_ref.backward(dz, y, scale, shift, mean, invstd, act, M)
                close(dy, yt.grad.numpy(), what + ' dy')
                close(dgamma, g.grad.numpy(), what + ' dgamma')
                close(dbeta, b.grad.numpy(), what + ' dbeta')
                close(c1 * M, dbeta, what + ' c1')
                close(c2 * M, dgamma, what + ' c2')
                if not with_res:
                    frozen = torch.from_numpy(y64).requires_grad_(True)
                    TORCH_ACT[act](frozen * torch.from_numpy(scale) + torch.from_numpy(shift)).backward(torch.from_numpy(dz.astype(np.float64)))
                    close(bn_ref.backward_frozen(dz, y, scale, shift, act), frozen.grad.numpy(), what + ' frozen dy')


def test_count_two_and_eval_coefficients_equal_torch():
    c = bc.finalize_inputs('count2')
    y = torch.from_numpy(c['y'].reshape(2, c['K']).astype(np.float64))
    rm, rv = torch.from_numpy(c['rm'].astype(np.float64)), torch.from_numpy(c['rv'].astype(np.float64))
    g, b = torch.from_numpy(c['gamma'].astype(np.float64)), torch.from_numpy(c['beta'].astype(np.float64))
    z = F.batch_norm(y, rm, rv, g, b, True, bc.MOMENTUM, bc.EPS)
    slabs = torch.stack([y.sum(0), (y * y).sum(0)])[None].numpy()
    scale, shift, _, _, rm1, rv1 = bn_ref.finalize(slabs, 2, c['gamma'], c['beta'], c['rm'], c['rv'], bc.EPS, bc.MOMENTUM)
    np.testing.assert_allclose(bn_ref.forward(y.numpy(), scale, shift, 0), z.numpy(), rtol=1e-9, atol=1e-9)    # var ~ 1e-2 from a difference of 1e0
    close(rm1, rm.numpy(), 'running_mean')
    np.testing.assert_allclose(rv1, rv.numpy(), rtol=1e-12)                                            # unbiased: twice the biased variance
    e = F.batch_norm(y, rm, rv, g, b, False, bc.MOMENTUM, bc.EPS)
    es, eh = bn_ref.eval_coeffs(c['gamma'], c['beta'], rm.numpy(), rv.numpy(), bc.EPS)
    close(y.numpy() * es + eh, e.numpy(), 'eval coefficients')


def test_sync_algebra_equals_one_rank_with_all_the_data():
    sets, counts, par = bc.sync_inputs()
    total = bn_ref.sync_sums(sets, counts)
    Ktot = bc.SYNC['Ktot']
    both = np.concatenate(sets).astype(np.float64).sum(0)
    close(total[:Ktot], both[0], 'sums')
    close(total[Ktot:2 * Ktot], both[1], 'square sums')
    assert total[2 * Ktot] == sum(counts)
    c1, c2 = bn_ref.sync_coeffs(total)
    close(c1, both[0] / sum(counts), 'c1')
    close(c2, both[1] / sum(counts), 'c2')


# ------------------------------------------------------------------------------------------ 2. what the cases contain
@pytest.mark.parametrize('name', list(bc.FINALIZE))
def test_finalize_case_contains_what_it_is_for(name):
    c = bc.finalize_inputs(name)
    K, k0, mt, count = c['K'], c['k0'], c['mtiles'], c['count']
    v = bc.finalize_view(c).astype(np.float64)
    assert v.shape == (mt, 2, K) and np.isfinite(v).all() and count == mt * c['rows']
    outside = np.delete(c['slabs'], np.arange(k0, k0 + K), axis=2)
    assert (outside == bc.POISON).all() and outside.shape[2] == c['stats_ld'] - K
    assert np.array_equal(v[:, 0], c['y'].sum(1, dtype=np.float32)) and len(np.unique(v[:, 0, 2])) >= mt - 2   # sums of data, no constants
    t = v.sum(0)
    raw = t[1] / count - (t[0] / count) ** 2
    scale, shift, mean, invstd, rm1, rv1 = bn_ref.finalize(v, count, c['gamma'], c['beta'], c['rm'], c['rv'], bc.EPS, bc.MOMENTUM)
    bounds = bn_ref.finalize_bounds(v, count, c['gamma'], c['beta'], c['rm'], c['rv'], bc.EPS, bc.MOMENTUM)
    assert raw[bc.CONST_CH] < 0 or (count <= 2 and raw[bc.CONST_CH] <= 0)                    # cancels below zero: the clamp decides invstd
    assert invstd[bc.CONST_CH] == 1.0 / np.sqrt(bc.EPS)
    if count >= 31 * 4:
        ratio = abs(mean[bc.FAR_CH]) / np.sqrt(raw[bc.FAR_CH])
        assert 0.8 * bc.FAR_RATIO < ratio < 1.25 * bc.FAR_RATIO, ratio
        assert (np.abs(v[-1, 0, 2:]) > 2 * np.abs(v[:-1, 0, 2:]).max(0)).all()               # the last slab stands out
    # a last slab counted twice moves every other channel's mean by at least 100 times the bound on the mean
    assert (np.abs(v[-1, 0, 2:]) / count >= 100 * bounds['mean'][2:]).all()
    if count == 1:
        assert (rv1 == (1 - bc.MOMENTUM) * c['rv'].astype(np.float64) + bc.MOMENTUM * np.maximum(raw, 0)).all()    # stays biased
    if count == 2:
        np.testing.assert_allclose(rv1 - (1 - bc.MOMENTUM) * c['rv'].astype(np.float64), bc.MOMENTUM * 2 * np.maximum(raw, 0), rtol=1e-9, atol=1e-15)
    clamped = bc.clamped_slots(mt)
    assert (clamped == 0) == (mt in (256, 1024)), clamped                                    # full batches of 256 slabs have no clamped slot
    if name.startswith('twostage'):
        assert mt > 1024 and bc.two_stage_groups(mt) == {1025: (33, 32), 1056: (33, 32), 2100: (66, 32)}[mt]
        tpg, groups = bc.two_stage_groups(mt)
        assert (mt - (groups - 1) * tpg == tpg) == (mt == 1056)                              # only 1056 fills its last group
        assert bc.clamped_slots(groups) == 7 * 32                                            # the final stage reads 32 partials: one live slot of 8 per lane
    if name.startswith('long'):
        assert mt > 1024 and not c['ws']
    if name == 'k20':
        assert K % 8 == 4
    if name == 'slice':
        assert (k0, K, c['stats_ld']) == (8, 24, 40)
    if name == 'pair':
        assert (c['Ka'], K, mt) == (8, 24, 257)
    assert K == 20 or K // 8 == 3


def test_forward_cases_contain_what_they_are_for():
    for dt in bc.DTYPES:
        ve = bc.VE[dt]
        k0, k1, k2, k3 = bc.FWD_K[dt]
        assert bc.chunks(k0, ve) == [1] and bc.chunks(k1, ve) == [k1 // ve]
        assert bc.chunks(k2, ve) == [256, 1] and bc.chunks(k3, ve) == [256, 12]
        assert bc.dead_lanes(12) == 4 and bc.dead_lanes(1) == 0 and bc.dead_lanes(k1 // ve) == 256 % (k1 // ve) > 0
        (Kb, on), (Kb2, off_), (Kn, Kan) = bc.PAIRS[dt]
        assert Kb == Kb2 == k3 and on == 256 * ve and off_ % ve == 0 and 0 < off_ < 256 * ve and off_ % (256 * ve) and Kan % ve == 0 and Kan < Kn
        y, _, scale, shift = bc.fwd_inputs(dt, k3, bc.SPECIAL_M, 'wide')
        u = y.astype(np.float64) * scale + shift
        assert u.min() == -100 and u.max() == 100 and (np.abs(u) < 1).any()
        y, _, scale, shift = bc.fwd_inputs(dt, k3, bc.SPECIAL_M, 'zeros')
        u = y.astype(np.float64) * scale + shift
        assert ((u == 0) & (y == 0)).sum() > 100 and ((u == 0) & (y == 1)).sum() > 100
        y, _, scale, shift = bc.fwd_inputs(dt, k3, bc.SPECIAL_M, 'nonfinite')
        for lo, hi in ((0, 256 * ve), (256 * ve, k3)):
            part = y[:, lo:hi]
            assert np.isnan(part).any() and (part == np.inf).any() and (part == -np.inf).any(), (dt, lo)
        for act in bc.ACTS:                                                                  # what each activation makes of them
            z = bn_ref.forward(y, scale, shift, act)
            assert np.array_equal(np.isnan(z), np.isnan(y) | ((act == bn_ref.ACT_SILU) & (y * scale == -np.inf)))
            if act == bn_ref.ACT_RELU:
                assert (z[y * scale == -np.inf] == 0).all() and (z[y * scale == np.inf] == np.inf).all()
        y, res, _, _ = bc.fwd_inputs(dt, k3, 257)
        assert np.array_equal(bc.rounded(y, dt), y) and np.array_equal(bc.rounded(res, dt), res)


def test_backward_cases_contain_what_they_are_for():
    assert [bc.bn_bwd_blocks(M) for M in (1, 34, 35, 64, 65, 150, 4000)] == [1, 1, 1, 1, 2, 3, 63]
    assert bc.rows_per_block(65) == 33 and bc.empty_blocks(65) == 0
    assert (bc.bn_bwd_blocks(32769), bc.rows_per_block(32769), bc.empty_blocks(32769)) == (512, 65, 7)
    dt, K, M = bc.BWD_FINALIZE_WIDE
    assert bc.bn_bwd_blocks(M) == 1024 and M * K * 2 <= 4 << 20 and bc.bn_bwd_blocks(M - 256) == 1023
    assert bc.chunks(1032, 4) == [256, 2] and bc.chunks(1072, 4) == [256, 12] and bc.chunks(1032, 8) == [129] and bc.dead_lanes(129) == 127
    # every residue mod 4 of a lane's row count (the four-row trips and their tail), for the 4-element kernels (fp32, reduce4) and the 8-element one
    for ve, cases in ((4, [c for c in bc.BWD]), (8, [c for c in bc.BWD if c[0] == 'bf16'])):
        seen = set()
        for _, K, M in cases:
            seen |= {n % 4 for n in bc.lane_rows(M, K, ve) if n > 0}
        assert seen == {0, 1, 2, 3}, (ve, seen)
        assert any(n >= 8 for _, K, M in cases for n in bc.lane_rows(M, K, ve))              # more than one full trip
    assert 0 in bc.lane_rows(32769, 48, 4)
    for n in bc.SLAB_COUNTS:
        assert bc.slab_inputs(n)[0].shape == (n, 2, bc.SLAB_K)
    assert [n >= 1024 for n in bc.SLAB_COUNTS] == [False, True, True, True] and bc.SLAB_K % 8 == 4
    assert bc.clamped_slots(1024, lanes=128) == 0 and bc.clamped_slots(1025, lanes=128) > 0 and bc.clamped_slots(1023, lanes=32) > 0


def test_yardstick_c_is_a_few_roundings():
    """c of bn_ref.sum_bound on every backward case: plain float32 loses a handful of roundings per term, 3.8 to 13.0 wherever a channel sums
    34 rows or more.  At M = 1 a sum is its one term and the worst of K channels sits next to the zero of silu' (u = -1.278), where the
    relative error of any float32 evaluation is large: c = 141 to 522 there, still 3e-5 of the term.  A yardstick beyond these limits would
    make the summation bound vacuous."""
    worst = {}
    for case in bc.BWD:
        for act in bc.BWD_ACTS:
            c = bn_ref.yardstick_c(*bc.bwd_inputs(*case), act)
            assert 1.0 <= c <= (16.0 if case[2] > 1 else 1024.0), (case, act, c)
            worst[act] = max(worst.get(act, 0.0), c)
    print('yardstick c, worst per activation:', worst)


# ------------------------------------------------------------------------------------------ 3. the comparers bite
def rejects(fn, *args):
    try:
        fn(*args)
    except AssertionError:
        return True
    return False


def test_comparers_reject_twice_the_bound_and_accept_half():
    c = bc.finalize_inputs('one-257')
    v = bc.finalize_view(c)
    args = (v, c['count'], c['gamma'], c['beta'], c['rm'], c['rv'], bc.EPS, bc.MOMENTUM)
    ref, bounds = bn_ref.finalize(*args), bn_ref.finalize_bounds(*args)
    assert bn_ref.check_finalize(ref, ref, bounds) == 0
    for i, name in enumerate(bn_ref.FINALIZE_NAMES):
        for k in (0, 1, 7, c['K'] - 1):
            for sign in (1, -1):
                half, twice = [a.copy() for a in ref], [a.copy() for a in ref]
                half[i][k] += sign * 0.5 * bounds[name][k]
                twice[i][k] += sign * 2 * bounds[name][k]
                assert 0.4 < bn_ref.check_finalize(half, ref, bounds) <= 0.6
                assert rejects(bn_ref.check_finalize, twice, ref, bounds), (name, k)
        assert (bounds[name] <= 4 * bn_ref.ULP * 1.001 * np.maximum(np.abs(ref[i]), 2.0)).all() or name in ('invstd', 'scale', 'shift')
    dz, y, scale, shift, mean, invstd = bc.bwd_inputs('bf16', 48, 150)
    du, dbeta, dgamma, c1, c2, dy = bn_ref.backward(dz, y, scale, shift, mean, invstd, bn_ref.ACT_SILU, 150)
    for bf16 in (False, True):
        b = bn_ref.elementwise_bound(dy, bf16)
        for idx in ((0, 0), (149, 47), tuple(np.unravel_index(np.argmin(np.abs(dy)), dy.shape)), tuple(np.unravel_index(np.argmax(np.abs(dy)), dy.shape))):
            half, twice = dy.copy(), dy.copy()
            half[idx] += 0.5 * b[idx]
            twice[idx] -= 2 * b[idx]
            assert 0.4 < bn_ref.check_elementwise(half, dy, bf16) <= 0.6
            assert rejects(bn_ref.check_elementwise, twice, dy, bf16)
        nan = dy.copy()
        nan[3, 3] = np.nan
        assert rejects(bn_ref.check_elementwise, nan, dy, bf16) and rejects(bn_ref.check_elementwise, dy, nan, bf16)
        assert bn_ref.check_elementwise(nan, nan, bf16) == 0
        inf = dy.copy()
        inf[3, 3] = np.inf
        assert rejects(bn_ref.check_elementwise, inf, dy, bf16) and rejects(bn_ref.check_elementwise, -inf, inf, bf16)
    a1, a2 = bn_ref.backward_abs_sums(dz, y, scale, shift, mean, invstd, bn_ref.ACT_SILU)
    for ref_v, a in ((dbeta, a1), (dgamma, a2)):
        b = bn_ref.sum_bound(a, bc.chain(150, 48, 4), 8.0)
        assert (b < 1e-4 * a).all()
        assert 0.4 < bn_ref.check_vector(ref_v + 0.5 * b, ref_v, b) <= 0.6
        for k in range(48):
            twice = ref_v.copy()
            twice[k] += 2 * b[k]
            assert rejects(bn_ref.check_vector, twice, ref_v, b)
