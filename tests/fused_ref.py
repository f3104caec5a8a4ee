"""Integer operands, float64 references and the launch geometry for the fused 1x1 backward (csrc/conv1x1_bwd.hip) and the two producers of
BatchNorm-backward statistics (hdy_conv1x1_bwd_fused_stats, hdy_conv_dgrad_stats); plain numpy / torch on the CPU, nothing here imports
hd_yolo_amd.  tests/test_fused_ref_host.py proves on the CPU what every case contains; tests/test_gpu_fused_exact.py runs them on the device.

The exact recipe.  The fused kernel takes scale, shift, mean, invstd, c1, c2 as independent inputs, so a case chooses (per channel k):

    dz, y, x   integers in [-2, 2]        dx0      integers in [-4, 4] (what an accumulating call finds in dx)
    mean, c1   integers in [-1, 1]        invstd   cycles through 1, 0.5, 2, -1       scale  cycles through 1, 1, -1, -1, 2, 2, -2, -2
    c2         j / invstd, j integer in [-1, 1]
    shift      24 + |scale| max|y|:  u = y scale + shift >= 24, where exp(-u) < 2^-25, 1 + exp(-u) rounds to 1 in fp32 and
               silu'(u) = s (1 + u (1 - s)) evaluates to exactly 1 (given rcp(1) == 1 on the device: the GPU file's probe asserts it first)
    W          [K][C], +-1 with probability pw = min(1, 80 / K), else 0  (or the identity)

Then du = dz, xhat = (y - mean) invstd is exact in both forms the kernels use, xhat c2 = (y - mean) j, and dy = scale (du - c1 - xhat c2)
is an integer with |dy| <= 12: exact in bf16, every product of the two GEMMs exact, every fp32 partial sum exact while SUM |term| < 2^24,
so dx, dW, every weight-gradient slab and every statistics slab are integers that depend on no summation order, tile order or grid.
For the statistics requests act = ACT_NONE makes du the stored bf16 dx itself and the unit tensors y_r are integers in [-2, 2].
`check_preconditions` asserts all of this on the reference; a case that violates it is an error in the test's design.

Geometry restated from the kernels (asserted against the library's own queries on the device):

    fused        BM = 128 rows per tile (64 for K >= 96), grid = min(tiles, 512), a workgroup walks tpb = ceil(tiles / grid) consecutive tiles;
                 workgroups past ceil(tiles / tpb) have none and write zero slabs.  Two x buffers, one in the 128-wide instance.
    igemm stat   BM = 128, column tile bn = 32 / 64, grid = min(256 * (4 at bn 32, 3 at bn 64), tiles); under the stride-2 class walk a tile
                 is (m-tile, parity class), four per m-tile.  Workgroup blockIdx owns position xcd_remap(blockIdx) of the contiguous ranges.

`chain`: the longest fp32 chain of a statistics launch.  A thread of the store loop owns one 16-byte channel chunk: CPR = C / 8 chunks per
row (bn / 8 in the igemm instances), RPI = 256 / CPR row lanes, so BM / RPI rows per tile and thread (fused C = 64: 4; igemm bn 64: 4,
bn 32: 2), added tile after tile in registers, then the RPI lanes through LDS: chain = (BM / RPI) * tiles per workgroup + RPI.
"""
import functools

import numpy as np
import torch

import bn_ref
import exact_ref

SUM_MAX = 2 ** 24
OUT_MAX = 256                      # integers up to here are exact in bf16
U_MIN = 24.0
INVSTD = (1.0, 0.5, 2.0, -1.0)
SCALE = (1.0, 1.0, -1.0, -1.0, 2.0, 2.0, -2.0, -2.0)
ACT_NONE, ACT_SILU = bn_ref.ACT_NONE, bn_ref.ACT_SILU
FUSED_K = (32, 64, 96, 128)
AXES_ROWS = ('row', 'channel')
AXES_DW = ('k', 'c')
AXES_SLAB = ('slab', 'stat', 'channel')


def cdiv(a, b):
    return -(-a // b)


def tile_rows(K):
    return 64 if K >= 96 else 128


def row_cases(K):
    """name -> M: the smallest row counts at which each path of the instance exists"""
    bm = tile_rows(K)
    return {'one': 1, 'tile-1': bm - 1, 'tile': bm, 'tile+1': bm + 1, 'few': 3 * bm + 37, 'two-tiles': 513 * bm + 5, 'three-tiles': 1025 * bm + 5}


# ------------------------------------------------------------------------------------------ geometry
def geometry(K, M):
    """hdy_conv1x1_bwd_fused_grid and the kernel's tile walk"""
    bm = tile_rows(K)
    tiles = cdiv(M, bm)
    grid = min(tiles, 512)
    tpb = cdiv(tiles, grid)
    working = cdiv(tiles, tpb)
    per_wg = [min(tpb, tiles - w * tpb) for w in range(working)]
    return dict(bm=bm, tiles=tiles, grid=grid, tpb=tpb, working=working, empty=grid - working, empty_slabs=list(range(working, grid)),
                last_rows=M - (tiles - 1) * bm, per_wg=sorted(set(per_wg)), xbufs=1 if K == 128 else 2, slabs=grid if K <= 64 else 0)


def xcd_remap(i, n):
    q, r, x, s = n >> 3, n & 7, i & 7, i >> 3
    return (x * (q + 1) if x < r else r * (q + 1) + (x - r) * q) + s


def igemm_geometry(N, H, W, C, stride):
    """the statistics instances of conv_igemm.hip serving a data gradient into [N][H][W][C]: igemm_grid and the contiguous tile ranges"""
    assert C <= 64 and stride in (1, 2)
    bn = 32 if C <= 32 else 64
    walk = stride == 2
    M = N * (H // 2) * (W // 2) if walk else N * H * W
    tiles = cdiv(M, 128) * (4 if walk else 1)
    grid = min(256 * (4 if bn == 32 else 3), tiles)
    tpb = cdiv(tiles, grid)
    working = cdiv(tiles, tpb)
    empty = [b for b in range(grid) if xcd_remap(b, grid) * tpb >= tiles]
    assert len(empty) == grid - working
    name = f'igemm_128x{bn}x2' + ('_walk' if walk else '') + '_stat'
    return dict(bn=bn, walk=walk, M=M, tiles=tiles, grid=grid, tpb=tpb, working=working, empty=grid - working, empty_slabs=empty,
                last_rows=M - (cdiv(M, 128) - 1) * 128, name=name)


def chain(kind, C, tpb):
    """the longest fp32 chain of a statistics launch (module docstring); kind 'fused' or 'igemm'"""
    bm = 128
    cpr = (C if kind == 'fused' else (32 if C <= 32 else 64)) // 8
    rpi = 256 // cpr
    return (bm // rpi) * tpb + rpi


# ------------------------------------------------------------------------------------------ the exact fused case
class Case:
    pass


def unit_tensor(M, width, seed):
    return np.random.RandomState(seed).randint(-2, 3, (M, width)).astype(np.float64)


def stat_expect(dx_final, requests, seed):
    """{(c0, c1): (y_r, SUM dx, SUM dx * y_r)} for the requests (c0, c1) over the final dx [M][C] (act none: du is dx itself)"""
    out = {}
    for c0, c1 in requests:
        y = unit_tensor(dx_final.shape[0], c1 - c0, seed + 31 * c0 + 977 * c1)
        d = dx_final[:, c0:c1]
        out[(c0, c1)] = (y, d.sum(0), (d * y).sum(0))
    return out


@functools.lru_cache(maxsize=2)
def fused_case(K, M, Ka=None, seed=0, requests=(), w='sparse'):
    """Operands and float64 results of one fused launch over M rows of K = C channels.  Ka only names where dz is cut into two tensors and dW
    into (dW_a, dW_b): the values do not depend on it.  Nothing in the returned case may be modified by a test (it is cached)."""
    rng = np.random.RandomState(100003 * K + M % 99991 + 7 * seed)
    c = Case()
    c.K = c.C = K
    c.M, c.Ka, c.requests, c.seed = M, Ka or K, tuple(requests), seed
    ints = lambda lo, hi, shape: rng.randint(lo, hi + 1, shape).astype(np.float64)
    c.dz, c.y, c.x, c.dx0 = ints(-2, 2, (M, K)), ints(-2, 2, (M, K)), ints(-2, 2, (M, K)), ints(-4, 4, (M, K))
    c.mean, c.c1, j = ints(-1, 1, K), ints(-1, 1, K), ints(-1, 1, K)
    c.invstd = np.array([INVSTD[k % 4] for k in range(K)])
    c.scale = np.array([SCALE[k % 8] for k in range(K)])
    c.c2 = j / c.invstd
    c.shift = U_MIN + np.abs(c.scale) * np.abs(c.y).max(0)
    if w == 'identity':
        c.pw, c.w = None, np.eye(K)
    else:
        c.pw = min(1.0, 80.0 / K)
        c.w = (rng.randint(0, 2, (K, K)) * 2.0 - 1.0) * (rng.random_sample((K, K)) < c.pw)
    c.u = c.y * c.scale + c.shift
    du, xhat = bn_ref.backward_terms(c.dz, c.y, c.scale, c.shift, c.mean, c.invstd, ACT_NONE)          # silu'(u) is 1 by construction
    c.dy = c.scale * (du - c.c1 - xhat * c.c2)
    c.dx = c.dy @ c.w
    c.dx_acc = c.dx + c.dx0
    c.dw = c.dy.T @ c.x
    c.dw_a, c.dw_b = c.dw[:c.Ka], c.dw[c.Ka:]
    c.stats = {acc: stat_expect(c.dx_acc if acc else c.dx, c.requests, seed) for acc in (False, True)}
    return c


def bf16_lossless(a):
    t = torch.from_numpy(np.ascontiguousarray(a, np.float64))
    return torch.equal(t.to(torch.bfloat16).double(), t)


def check_preconditions(c):
    """The conditions under which every leg of the case is exact, on the reference alone.  They are not skips."""
    tag = f'K {c.K} M {c.M}'
    for name in ('dz', 'y', 'x', 'dx0', 'w', 'dy', 'dx', 'dx_acc'):
        assert bf16_lossless(getattr(c, name)), f'{tag}: {name} is not exact in bf16'
    for name in ('scale', 'shift', 'mean', 'invstd', 'c1', 'c2'):
        a = getattr(c, name)
        assert np.array_equal(a.astype(np.float32).astype(np.float64), a), f'{tag}: {name} is not exact in fp32'
    m, e = np.frexp(np.abs(np.concatenate([c.scale, c.invstd])))
    assert (m == 0.5).all(), f'{tag}: scale / invstd are not powers of two'
    assert np.array_equal(c.c2 * c.invstd, np.round(c.c2 * c.invstd)), f'{tag}: c2 is no multiple of 1 / invstd'
    assert c.u.min() >= U_MIN, f'{tag}: min u = {c.u.min()} < {U_MIN}: silu\' would not be exactly 1'
    for name in ('dy', 'dx', 'dw'):
        assert np.array_equal(getattr(c, name), np.round(getattr(c, name))), f'{tag}: {name} is not integer'
    dymax, dxmax = np.abs(c.dy).max(), (np.abs(c.dx) + np.abs(c.dx0)).max()
    assert dymax <= OUT_MAX, f'{tag}: max |dy| = {dymax}'
    assert dxmax <= OUT_MAX, f'{tag}: max |dx| + |dx0| = {dxmax}: the accumulated data gradient would round in bf16'
    s_dw = (np.abs(c.dy).T @ np.abs(c.x)).max()
    s_dx = (np.abs(c.dx) + np.abs(c.dx0)).sum(0).max()
    assert s_dw < SUM_MAX, f'{tag}: SUM |dy x| = {s_dw} >= 2^24'
    assert s_dx < SUM_MAX, f'{tag}: SUM |dx| = {s_dx} >= 2^24'
    s_st = 0.0
    for (c0, c1), (y, _, _) in c.stats[True].items():
        s_st = max(s_st, ((np.abs(c.dx[:, c0:c1]) + np.abs(c.dx0[:, c0:c1])) * np.abs(y)).sum(0).max())
    assert s_st < SUM_MAX, f'{tag}: SUM |dx y_r| = {s_st} >= 2^24'
    assert (np.abs(c.w).sum(0) > 0).all() and (np.abs(c.w).sum(1) > 0).all(), f'{tag}: a filter row or column is all zero'
    return dict(dymax=dymax, dxmax=dxmax, sum_dw=s_dw / SUM_MAX, sum_dx=s_dx / SUM_MAX, sum_stat=s_st / SUM_MAX, umin=c.u.min(),
                distinct_dx=len(np.unique(c.dx[:4096])))


def kernel_formula_f32(dz, y, scale, shift, mean, invstd, c1, c2, act=ACT_SILU):
    """The element-wise phase of conv1x1_bwd.hip literally, in numpy float32 (an fma is the float64 value rounded once: exact for a product
    of two fp32 numbers plus a third up to one rounding):  u = fma(y, scale, shift);  s = 1 / (1 + exp2(u * -log2 e));
    du = dz * (s * fma(u, 1 - s, 1));  xhat = fma(y, invstd, -mean * invstd);  d = scale * fma(xhat, -c2, du - c1).  fp32 [M][K], not yet bf16."""
    f, d64 = np.float32, np.float64
    dz, y, sc, sh, mu, inv, k1, k2 = (np.asarray(a, f) for a in (dz, y, scale, shift, mean, invstd, c1, c2))
    fma = lambda a, b, c: (a.astype(d64) * b.astype(d64) + c.astype(d64)).astype(f)
    u = fma(y, sc, sh)
    if act == ACT_SILU:
        with np.errstate(over='ignore'):
            t = np.exp2(u * f(-1.4426950408889634)).astype(f) + f(1)
        s = f(1) / t
        du = dz * (s * fma(u, f(1) - s, np.ones_like(u)))
    else:
        du = dz
    xhat = fma(y, inv, -mu * inv)
    out = sc * fma(xhat, -k2, du - k1)
    assert out.dtype == f
    return out


def to_bf16(a):
    """fp32 / fp64 array rounded to the nearest bf16, as float64"""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).double().numpy()


# ------------------------------------------------------------------------------------------ the data gradient with statistics
@functools.lru_cache(maxsize=2)
def dgrad_stat_case(N, H, W, C, K, R, stride, pad, requests, seed=0):
    """hdy_conv_dgrad_stats into dx [N][H][W][C] from dy with K channels: exact_ref.reference for the operands and dx, integer unit tensors
    and the exact column sums of the final dx per request, written and accumulated (exact_ref's dx_acc is what the accumulating call finds)."""
    e = exact_ref.reference((N, H, W, C, K, R, stride, pad))
    c = Case()
    c.e, c.case, c.requests = e, (N, H, W, C, K, R, stride, pad), tuple(requests)
    c.M = N * H * W
    c.dx = exact_ref.nhwc(e.dx).reshape(c.M, C).numpy()
    c.dx0 = exact_ref.nhwc(e.dx_acc).reshape(c.M, C).numpy()
    c.dx_acc = c.dx + c.dx0
    c.stats = {acc: stat_expect(c.dx_acc if acc else c.dx, c.requests, seed + 1000) for acc in (False, True)}
    return c


def check_dgrad_preconditions(c):
    tag = str(c.case)
    assert np.array_equal(c.dx, np.round(c.dx)) and bf16_lossless(c.dx) and bf16_lossless(c.dx_acc), f'{tag}: dx is not an integer exact in bf16'
    dxmax = (np.abs(c.dx) + np.abs(c.dx0)).max()
    assert dxmax <= OUT_MAX, f'{tag}: max |dx| + |dx0| = {dxmax}'
    assert bool((c.e.w.abs().sum((0, 2, 3)) > 0).all()) and bool((c.e.w.abs().sum((1, 2, 3)) > 0).all()), f'{tag}: an all-zero filter'
    s1 = (np.abs(c.dx) + np.abs(c.dx0)).sum(0).max()
    s2 = 0.0
    for (c0, c1), (y, _, _) in c.stats[True].items():
        s2 = max(s2, ((np.abs(c.dx[:, c0:c1]) + np.abs(c.dx0[:, c0:c1])) * np.abs(y)).sum(0).max())
    assert s1 < SUM_MAX and s2 < SUM_MAX, f'{tag}: SUM |dx| = {s1}, SUM |dx y_r| = {s2}: a slab sum would round'
    return dict(dxmax=dxmax, sum_dx=s1 / SUM_MAX, sum_stat=s2 / SUM_MAX)


def request_shapes(C):
    """all of dx; two units with the boundary off C / 2; one unit that leaves the first and the last chunk to no request"""
    return {'whole': ((0, C),), 'split8': ((0, 8), (8, C)), 'inner': ((8, C - 8),)}


def all_requests(C):
    """every distinct range of request_shapes: a case built with these serves the three shapes"""
    return tuple(sorted({r for shape in request_shapes(C).values() for r in shape}))


# ------------------------------------------------------------------------------------------ slab comparer
def assert_slabs_exact(slabs, want_s1, want_s2, empty_slabs, what):
    """slabs: fp32 [n][2][w] as the kernel wrote them over a NaN prefill.  Every slab written, every value an integer, the slabs of the
    workgroups without tiles exactly 0, and the float64 sum over slabs EQUAL to the integer column sums of the reference."""
    slabs = slabs.detach().cpu()
    bad = (~torch.isfinite(slabs)).flatten(1).any(1).nonzero().flatten().tolist()
    assert not bad, f'{what}: {len(bad)} of {slabs.shape[0]} statistic slabs hold a non-finite value (never written), the first ones {bad[:8]}'
    assert torch.equal(slabs, slabs.round()), f'{what}: a slab holds a non-integer'
    if empty_slabs:
        nz = [s for s in empty_slabs if slabs[s].abs().max() != 0]
        assert not nz, f'{what}: slabs of workgroups without tiles are not zero: {nz[:8]}'
    total = slabs.double().sum(0, keepdim=True)
    want = torch.from_numpy(np.stack([want_s1, want_s2]))[None]
    exact_ref.assert_exact(total, want, f'{what} (slab 0 = the sum of all {slabs.shape[0]} slabs)', AXES_SLAB)


# ------------------------------------------------------------------------------------------ real-valued legs
def dy_reference(dz, y, scale, shift, mean, invstd, c1_32, c2_32, act=ACT_SILU):
    """float64 dy = scale (du - c1 - xhat c2) from the operands as the kernel receives them (c1 / c2: the fp32 values actually passed)"""
    du, xhat = bn_ref.backward_terms(dz, y, scale, shift, mean, invstd, act)
    return bn_ref.f64(scale) * (du - bn_ref.f64(c1_32) - xhat * bn_ref.f64(c2_32))


def real_coeffs(inputs, act=ACT_SILU):
    """c1 / c2 of the float64 backward over the inputs of bn_cases.bwd_inputs, cast to fp32 as the reduce + finalize launches leave them"""
    r = bn_ref.backward(*inputs, act, inputs[0].shape[0])
    return r[3].astype(np.float32), r[4].astype(np.float32)


def stat_terms(dx_bits, y_r, scale_r, shift_r, act):
    """(du, du * y) in float64: du = dx * act'(y scale + shift) from the dx values read back"""
    dx, y = bn_ref.f64(dx_bits), bn_ref.f64(y_r)
    du = dx * bn_ref.act_grad(y * bn_ref.f64(scale_r) + bn_ref.f64(shift_r), act)
    return du, du * y


def stat_sums_reference(dx_bits, y_r, scale_r, shift_r, act):
    """((SUM du, SUM du y), (SUM |du|, SUM |du y|)) per channel"""
    du, duy = stat_terms(dx_bits, y_r, scale_r, shift_r, act)
    return (du.sum(0), duy.sum(0)), (np.abs(du).sum(0), np.abs(duy).sum(0))


def yardstick(dx_bits, y_r, scale_r, shift_r, act):
    """`c` of bn_ref.sum_bound for the pair (du, du * y), in the manner of bn_ref.yardstick_c: the same two terms in plain float32 (numpy exp and
    division), per channel SUM |term32 - term64| / SUM |term64|, the worst channel of the two sums, times four, in units of 2^-24, plus 1 for the
    cast of the finished sum."""
    f = np.float32
    dx, y, sc, sh = (np.asarray(a, f) for a in (dx_bits, y_r, scale_r, shift_r))
    du64, duy64 = stat_terms(dx_bits, y_r, scale_r, shift_r, act)
    if act == ACT_SILU:
        u = y * sc + sh
        with np.errstate(over='ignore'):
            s = f(1) / (f(1) + np.exp(-u))
        du32 = dx * (s * (f(1) + u * (f(1) - s)))
    else:
        du32 = dx
    worst = 0.0
    for t32, t64 in ((du32, du64), (du32 * y, duy64)):
        assert t32.dtype == f
        den, num = np.abs(t64).sum(0), np.abs(bn_ref.f64(t32) - t64).sum(0)
        worst = max(worst, float(np.max(np.where(den > 0, num / np.maximum(den, 1e-300), 0.0))))
    return 4.0 * worst / bn_ref.U32 + 1.0


# ------------------------------------------------------------------------------------------ case lists
EXACT = [(K, name) for K in FUSED_K for name in row_cases(K)]
STAT_K = (32, 64)
STAT_ROWS = ('tile+1', 'two-tiles', 'three-tiles')
# hdy_conv_dgrad_stats (N, H, W, C, K, R, stride, pad).  The two long ones are the smallest launches in which a workgroup of a statistics instance
# takes a second tile: 128 * grid + 5 output pixels (grid 1024 at bn 32, 768 at bn 64), as N rows of W pixels because the loader addresses image
# sides below 24000 (131205 = 15 * 8747, 98437 = 173 * 569)
DGRAD = {'1x1': (2, 24, 20, 64, 32, 1, 1, 0), '3x3': (3, 16, 16, 32, 64, 3, 1, 1), 's2-walk': (2, 16, 24, 64, 128, 3, 2, 1),
         'long-bn32': (15, 1, 8747, 32, 8, 1, 1, 0), 'long-bn64': (173, 1, 569, 64, 8, 1, 1, 0)}
REAL_ROWS = ('tile+1', 'few')


def partition_slabs(dx_final, y_r, c0, c1, bm, tpb, grid):
    """float32 [grid][2][c1 - c0]: the slabs a launch leaves when workgroup w sums the rows of its tiles [w tpb, (w + 1) tpb)"""
    M = dx_final.shape[0]
    out = np.zeros((grid, 2, c1 - c0), np.float32)
    d = dx_final[:, c0:c1]
    for w in range(grid):
        lo, hi = min(w * tpb * bm, M), min((w + 1) * tpb * bm, M)
        out[w, 0], out[w, 1] = d[lo:hi].sum(0), (d[lo:hi] * y_r[lo:hi]).sum(0)
    return torch.from_numpy(out)
