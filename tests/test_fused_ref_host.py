"""CPU side of the exact tests of the fused 1x1 backward and the statistics producers (tests/fused_ref.py):

1. every case passes the preconditions of the integer recipe and contains what its name claims (partial last tile, a single row,
   workgroups with 2 and with 3 tiles, workgroups without tiles, a request boundary off C / 2, a chunk of dx that belongs to no request);
2. a literal fp32 evaluation of the kernel's element-wise formula reproduces dy BIT FOR BIT on every exact case: the construction, and not
   the kernel, is exact;
3. on the real-valued inputs the same fp32 formula sits well inside the criterion the kernel is then held to;
4. the comparers reject, with the right coordinates, the seven errors the data movement of these kernels can make.

On (3): a bf16 output cannot stay within HALF of bn_ref.elementwise_bound(ref, bf16=True) = (1e-4 + 2^-8) |ref| + 0.2e-4 rms: rounding to
bf16 alone costs up to 2^-8 |ref|, 0.975 of that bound (tests/test_gpu_bn_direct.py: "a bf16 output sits at 0.97 by construction").  What
is asserted is the part that can hold and asks more of the arithmetic: the fp32 value BEFORE the rounding stays within half of the fp32
bound (1e-4 |ref| + 0.2e-4 rms; measured 0.006 at most), and after the rounding within the bf16 bound (measured 0.943 to 0.968).
"""
import numpy as np
import pytest
import torch

import bn_cases as bc
import bn_ref
import exact_ref as X
import fused_ref as F
from test_exact_host import rejected


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64))


def as_bf16(a):
    return t64(a).to(torch.bfloat16)


# ------------------------------------------------------------------------------------------ 1, 2: the exact cases
@pytest.mark.parametrize('K,name', F.EXACT, ids=[f'{K}-{n}' for K, n in F.EXACT])
def test_exact_case_holds_its_preconditions_and_the_fp32_formula_reproduces_dy(K, name):
    M = F.row_cases(K)[name]
    c = F.fused_case(K, M)
    r = F.check_preconditions(c)
    assert r['dymax'] <= 12 and (M < 64 or r['distinct_dx'] >= 32), r
    got = F.kernel_formula_f32(c.dz, c.y, c.scale, c.shift, c.mean, c.invstd, c.c1, c.c2)
    assert np.array_equal(got.view(np.int32), c.dy.astype(np.float32).view(np.int32)), f'K {K} M {M}: the fp32 formula does not give dy bit for bit'
    X.lossless(t64(c.dy), torch.bfloat16), X.lossless(t64(c.dx_acc), torch.bfloat16), X.lossless(t64(c.dw), torch.float32)
    assert np.abs(c.dx).max() > 0 and np.abs(c.dw).max() > 0 and len(np.unique(c.scale)) == 4 and len(np.unique(c.invstd)) == 4


def test_identity_case_copies_dy():
    c = F.fused_case(64, 130, w='identity')
    F.check_preconditions(c)
    assert np.array_equal(c.dx, c.dy)


def test_the_silu_derivative_saturates_to_one_in_fp32():
    """s (1 + u (1 - s)) == 1 in numpy float32 for every fp32 u in [24, 200) on a fine grid, with the kernel's exp2 argument"""
    u = np.concatenate([np.linspace(24, 200, 2000001), np.arange(24, 200, 0.5)]).astype(np.float32)
    t = np.exp2(u * np.float32(-1.4426950408889634)).astype(np.float32) + np.float32(1)
    s = np.float32(1) / t
    assert (t == 1).all() and (s * (np.float32(1) + u * (np.float32(1) - s)) == 1).all()


def test_geometry_shows_what_the_row_cases_claim():
    for K in F.FUSED_K:
        bm, rows = F.tile_rows(K), F.row_cases(K)
        g = {n: F.geometry(K, M) for n, M in rows.items()}
        assert bm == (128 if K <= 64 else 64)
        assert g['one']['tiles'] == 1 and g['one']['last_rows'] == 1 and g['one']['grid'] == 1
        assert g['tile-1']['last_rows'] == bm - 1 and g['tile']['last_rows'] == bm and g['tile']['tiles'] == 1
        assert g['tile+1']['tiles'] == 2 and g['tile+1']['last_rows'] == 1
        assert g['few']['tiles'] == 4 and g['few']['per_wg'] == [1] and g['few']['last_rows'] == 37 and g['few']['empty'] == 0
        two, three = g['two-tiles'], g['three-tiles']
        assert two['grid'] == 512 and two['tpb'] == 2 and two['per_wg'] == [2] and two['empty'] == 255 and two['last_rows'] == 5
        assert three['grid'] == 512 and three['tpb'] == 3 and three['per_wg'] == [3] and three['empty'] == 170 and three['last_rows'] == 5
        # one tile fewer and no workgroup takes a second (third) tile: the smallest such launches
        assert F.geometry(K, rows['two-tiles'] - 5 - bm)['tpb'] == 1 and F.geometry(K, rows['three-tiles'] - 5 - bm)['tpb'] == 2
        assert (two['slabs'] == 512) == (K <= 64) and g['one']['xbufs'] == (1 if K == 128 else 2)
    assert rows['three-tiles'] == 65605 and F.row_cases(64)['three-tiles'] == 131205


def test_request_shapes_have_an_odd_boundary_and_an_unserved_chunk():
    for C in F.STAT_K:
        s = F.request_shapes(C)
        assert s['whole'] == ((0, C),)
        assert s['split8'][0][1] == s['split8'][1][0] == 8 != C // 2
        (c0, c1), = s['inner']
        assert c0 == 8 and c1 == C - 8 and c1 > c0                 # chunks [0, 8) and [C - 8, C) belong to no request
        assert all(a % 8 == 0 and b % 8 == 0 for shape in s.values() for a, b in shape)
        assert set(F.all_requests(C)) == {(0, C), (0, 8), (8, C), (8, C - 8)}


@pytest.mark.parametrize('K,name', [(K, n) for K in F.STAT_K for n in F.STAT_ROWS], ids=lambda v: str(v))
def test_statistics_cases_hold_their_preconditions(K, name):
    M = F.row_cases(K)[name]
    c = F.fused_case(K, M, requests=F.all_requests(K))
    r = F.check_preconditions(c)
    assert 0 < r['sum_stat'] < 1 and 0 < r['sum_dx'] < 1
    g = F.geometry(K, M)
    for acc in (False, True):
        final = c.dx_acc if acc else c.dx
        for (c0, c1), (y, s1, s2) in c.stats[acc].items():
            assert np.array_equal(s1, np.round(s1)) and np.array_equal(s2, np.round(s2)) and np.abs(s2).max() > 0
            slabs = F.partition_slabs(final, y, c0, c1, g['bm'], g['tpb'], g['grid'])
            F.assert_slabs_exact(slabs, s1, s2, g['empty_slabs'], f'K {K} M {M} [{c0}, {c1}) acc {acc}')
            assert (slabs[g['working'] - 1].abs().max() > 0) and (g['empty'] == 0 or slabs[g['working']].abs().max() == 0)


@pytest.mark.parametrize('name', list(F.DGRAD))
def test_data_gradient_cases_hold_their_preconditions(name):
    case = F.DGRAD[name]
    N, H, W, C, K, R, stride, pad = case
    c = F.dgrad_stat_case(*case, F.all_requests(C))
    F.check_dgrad_preconditions(c)
    g = F.igemm_geometry(N, H, W, C, stride)
    assert g['name'] == {'1x1': 'igemm_128x64x2_stat', '3x3': 'igemm_128x32x2_stat', 's2-walk': 'igemm_128x64x2_walk_stat',
                         'long-bn32': 'igemm_128x32x2_stat', 'long-bn64': 'igemm_128x64x2_stat'}[name]
    if name.startswith('long'):
        # the smallest launch in which a workgroup of this instance takes a second tile, with a partial last tile and workgroups without tiles
        assert g['tiles'] > g['grid'] == (1024 if C == 32 else 768) and g['tpb'] == 2 and g['last_rows'] == 5 and g['empty'] > 0
        assert F.igemm_geometry(1, 1, 128 * g['grid'], C, 1)['tpb'] == 1 and g['tiles'] == g['grid'] + 2
        assert max(H, W) < 24000
    else:
        assert g['tpb'] == 1 and g['empty'] == 0 and g['grid'] == g['tiles']
    if name == 's2-walk':
        assert g['walk'] and g['tiles'] == 4 * F.cdiv(N * (H // 2) * (W // 2), 128) and H % 2 == 0 and W % 2 == 0


def test_chain_follows_the_kernels_constants():
    assert F.chain('fused', 64, 2) == 4 * 2 + 32 and F.chain('fused', 32, 3) == 2 * 3 + 64
    assert F.chain('igemm', 64, 1) == 4 + 32 and F.chain('igemm', 32, 2) == 2 * 2 + 64 and F.chain('igemm', 16, 1) == 2 + 64


# ------------------------------------------------------------------------------------------ 3: the real-valued inputs
@pytest.mark.parametrize('K', F.FUSED_K)
@pytest.mark.parametrize('name', F.REAL_ROWS)
def test_fp32_formula_sits_inside_the_criterion_on_the_real_valued_inputs(K, name):
    M = F.row_cases(K)[name]
    inputs = bc.bwd_inputs('bf16', K, M)
    c1, c2 = F.real_coeffs(inputs)
    ref = F.dy_reference(*inputs, c1, c2)
    got32 = F.kernel_formula_f32(*inputs, c1, c2)
    before = bn_ref.check_elementwise(got32, ref, False, f'K {K} M {M} fp32')
    after = bn_ref.check_elementwise(F.to_bf16(got32), ref, True, f'K {K} M {M} bf16')
    print(f'F1HOST {K}-{M} | fp32 {before:.4f} | bf16 {after:.4f}')
    assert before <= 0.5 and after <= 1.0
    assert np.abs(ref).max() > 0.5 and np.isfinite(ref).all()


def test_yardstick_and_reference_sums_of_the_statistics_terms():
    rng = np.random.RandomState(3)
    dx = F.to_bf16(rng.uniform(-1, 1, (300, 16)))
    y = F.to_bf16(rng.standard_normal((300, 16)) * 1.2 + 0.3)
    scale, shift = bc.coeffs(16)
    (s1, s2), (a1, a2) = F.stat_sums_reference(dx, y, scale, shift, F.ACT_SILU)
    du = dx * bn_ref.act_grad(y * scale.astype(np.float64) + shift.astype(np.float64), F.ACT_SILU)
    assert np.allclose(s1, du.sum(0), rtol=0, atol=1e-12) and np.allclose(s2, (du * y).sum(0), rtol=0, atol=1e-12)
    assert (a1 >= np.abs(s1)).all() and (a2 >= np.abs(s2)).all()
    assert 1.0 < F.yardstick(dx, y, scale, shift, F.ACT_SILU) < 40.0
    assert F.yardstick(dx, y, scale, shift, F.ACT_NONE) < 3.0          # du is dx itself: only the product rounds


# ------------------------------------------------------------------------------------------ 4: mutations
K_MUT, M_MUT = 64, 3 * 128 + 37
TILE = 128


def mutation_case():
    return F.fused_case(K_MUT, M_MUT, requests=F.all_requests(K_MUT))


def dx_rejected(dx):
    c = mutation_case()
    return rejected(lambda: X.assert_exact(as_bf16(dx), t64(c.dx), 'dx', F.AXES_ROWS))


def dw_rejected(dw):
    c = mutation_case()
    return rejected(lambda: X.assert_exact(t64(dw).float(), t64(c.dw), 'dW', F.AXES_DW))


def test_the_unmutated_reference_passes():
    c = mutation_case()
    assert dx_rejected(c.dx) is None and dw_rejected(c.dw) is None


def test_two_rows_of_a_tile_swapped():
    """a wrong swizzle: rows 9 and 10 of tile 1"""
    c = mutation_case()
    dx = c.dx.copy()
    dx[[TILE + 9, TILE + 10]] = dx[[TILE + 10, TILE + 9]]
    msg = dx_rejected(dx)
    assert msg and f'row {TILE + 9}..{TILE + 10}' in msg


def test_the_two_halves_of_a_16_byte_chunk_swapped():
    """the skey parity: channels [16, 20) and [20, 24) of one row"""
    c = mutation_case()
    dx = c.dx.copy()
    row = 2 * TILE + 5
    dx[row, 16:24] = np.concatenate([c.dx[row, 20:24], c.dx[row, 16:20]])
    msg = dx_rejected(dx)
    assert not np.array_equal(dx[row, 16:24], c.dx[row, 16:24])
    assert msg and f'row {row}..{row}' in msg and 'channel 1' in msg and 'channel 0' not in msg


def test_the_dz_split_moved_by_eight_channels():
    """the kernel reading with Ka + 8: chunk Ka comes from beyond dz_a's width (the buffer's 7.0), every later chunk from 8 channels before"""
    c = mutation_case()
    Ka = K_MUT // 2
    dz = c.dz.copy()
    dz[:, Ka:Ka + 8] = bc.POISON
    dz[:, Ka + 8:] = c.dz[:, Ka:-8]
    du, xhat = bn_ref.backward_terms(dz, c.y, c.scale, c.shift, c.mean, c.invstd, F.ACT_NONE)
    dy = c.scale * (du - c.c1 - xhat * c.c2)
    assert not np.array_equal(dy[:, Ka:], c.dy[:, Ka:]) and np.array_equal(dy[:, :Ka], c.dy[:, :Ka])
    assert dx_rejected(dy @ c.w) and dw_rejected(dy.T @ c.x)
    # and on the gradient side: grad_a of Ka + 8 rows next to grad_b shows as rows of dW out of place
    moved = np.concatenate([c.dw[:Ka], c.dw[Ka + 8:], c.dw[Ka:Ka + 8]])
    msg = dw_rejected(moved)
    assert msg and f'k {Ka}..' in msg


def test_the_last_row_of_a_partial_tile_contributing_to_dw():
    """row M of the last tile (a masked row) read as a copy of row M - 1"""
    c = mutation_case()
    dw = c.dw + np.outer(c.dy[-1], c.x[-1])
    assert np.abs(dw - c.dw).max() <= 24                                   # far below 1.5e-2 of the largest element's sum over 421 rows
    assert dw_rejected(dw)


def stat_slabs(c, acc, rng_req):
    g = F.geometry(K_MUT, M_MUT)
    y, s1, s2 = c.stats[acc][rng_req]
    final = c.dx_acc if acc else c.dx
    return g, y, s1, s2, F.partition_slabs(final, y, *rng_req, g['bm'], g['tpb'], g['grid'])


def test_one_pixel_counted_twice_in_a_slab():
    c = mutation_case()
    req = (8, K_MUT)
    g, y, s1, s2, slabs = stat_slabs(c, True, req)
    assert rejected(lambda: F.assert_slabs_exact(slabs, s1, s2, g['empty_slabs'], 'slabs')) is None
    row = TILE + 127                                                       # the last row of tile 1
    s = slabs.clone()
    s[1, 0] += torch.from_numpy(c.dx_acc[row, req[0]:req[1]]).float()
    s[1, 1] += torch.from_numpy(c.dx_acc[row, req[0]:req[1]] * y[row]).float()
    msg = rejected(lambda: F.assert_slabs_exact(s, s1, s2, g['empty_slabs'], 'slabs'))
    assert msg and 'elements differ' in msg
    one = slabs.clone()                                                    # one channel of one row, in the product row only
    k = int(np.argmax(np.abs(c.dx_acc[row, req[0]:req[1]] * y[row])))
    one[1, 1, k] += float(c.dx_acc[row, req[0] + k] * y[row, k])
    msg = rejected(lambda: F.assert_slabs_exact(one, s1, s2, g['empty_slabs'], 'slabs'))
    assert msg and '1 of' in msg and f'channel {k}..{k}' in msg


def test_one_slab_left_unwritten():
    c = mutation_case()
    g, y, s1, s2, slabs = stat_slabs(c, False, (0, K_MUT))
    s = slabs.clone()
    s[2] = float('nan')
    msg = rejected(lambda: F.assert_slabs_exact(s, s1, s2, g['empty_slabs'], 'slabs'))
    assert msg and 'never written' in msg and '[2]' in msg
    # a slab of a workgroup without tiles that keeps an earlier launch's finite values
    big = F.geometry(64, F.row_cases(64)['two-tiles'])
    stale = torch.zeros((big['grid'], 2, 8))
    stale[big['working'] + 3] = 1.0
    msg = rejected(lambda: F.assert_slabs_exact(stale, np.zeros(8), np.zeros(8), big['empty_slabs'], 'slabs'))
    assert msg and 'without tiles' in msg and str(big['working'] + 3) in msg


def test_the_first_tiles_x_used_for_the_third_tile():
    """buffer parity: a workgroup that walks three tiles finds its first x tile again in buffer 0"""
    c = mutation_case()
    x = c.x.copy()
    x[2 * TILE:3 * TILE] = c.x[0:TILE]
    dw = c.dy.T @ x
    msg = dw_rejected(dw)
    assert msg and 'k 0..63' in msg and 'c 0..63' in msg
