"""The cases of the direct tests of csrc/bn_act.hip, shared by test_bn_ref_host.py (which proves on the CPU that every case contains what
its name claims) and test_gpu_bn_direct.py.  Everything is generated, as exact float32 values (bf16 cases: values a bf16 holds exactly);
nothing here imports hd_yolo_amd.  Each case is the smallest tensor that reaches the named path of the kernels; the launch geometry of
bn_act.hip (row blocks, column chunks, lane_map, the two-stage finalize) is restated here in Python so that this can be asserted.
"""
import functools
import math

import numpy as np
import torch

import bn_ref

F32 = np.float32
EPS, MOMENTUM = float(F32(1e-3)), float(F32(0.03))        # what the kernels receive: ops.BN_EPS / BN_MOMENTUM as C floats
DTYPES = ('f32', 'bf16')
VE = {'f32': 4, 'bf16': 8}                                  # elements of one 16-byte vector
TORCH = {'f32': torch.float32, 'bf16': torch.bfloat16}
POISON = 7.0


def rounded(a, dt):
    """float32 array of values the arithmetic type holds exactly"""
    a = np.ascontiguousarray(a, F32)
    return torch.from_numpy(a).to(torch.bfloat16).float().numpy() if dt == 'bf16' else a


# ------------------------------------------------------------------------------------------ geometry of bn_act.hip, restated
def cdiv(a, b):
    return -(-a // b)


def bn_bwd_blocks(M):
    """hdy_bn_bwd_blocks: 256+ rows per block and at most 1024 blocks for large tensors, down to 64 rows per block for small ones"""
    return max(min(cdiv(M, 256), 1024), min(cdiv(M, 64), 512), 1)


def rows_per_block(M):
    return cdiv(M, bn_bwd_blocks(M))


def empty_blocks(M):
    nb, rows = bn_bwd_blocks(M), rows_per_block(M)
    return sum(1 for b in range(nb) if b * rows >= M)


def chunks(K, ve):
    """lane_map: vectors per row in every column chunk of 256 lane-vectors"""
    vct = K // ve
    return [min(256, vct - c * 256) for c in range(cdiv(vct, 256))]


def dead_lanes(vc):
    """lanes of a 256-thread workgroup with rl >= RL = 256 / VC"""
    return 256 - (256 // vc) * vc


def lane_rows(M, K, ve):
    """every number of rows a live lane of the reduce kernels sums, over all blocks, chunks and row lanes"""
    rows, out = rows_per_block(M), set()
    for b in range(bn_bwd_blocks(M)):
        n = max(min((b + 1) * rows, M) - b * rows, 0)
        for vc in chunks(K, ve):
            RL = 256 // vc
            out |= {max(cdiv(n - rl, RL), 0) for rl in range(RL)}
    return out


def chain(M, K, ve):
    """`n` of bn_ref.sum_bound: the longest fp32 chain, a lane's rows plus the workgroup's RL row lanes"""
    rows = rows_per_block(M)
    return max(cdiv(rows, 256 // vc) + 256 // vc for vc in chunks(K, ve))


def two_stage_groups(mtiles):
    """bn_partial_kernel: 32 groups of cdiv(mtiles, 32) slabs; (slabs per group, groups the final stage reads)"""
    tpg = cdiv(mtiles, 32)
    return tpg, cdiv(mtiles, tpg)


def clamped_slots(mtiles, lanes=32):
    """bn_finalize_kernel: slots of the 8-per-lane batches that fall past the last slab (clamped to it and weighted 0)"""
    n = 0
    for tl in range(lanes):
        for t in range(tl, mtiles, 8 * lanes):
            n += sum(1 for u in range(8) if t + lanes * u >= mtiles)
    return n


# ------------------------------------------------------------------------------------------ finalize
def _fin(mtiles, K=24, ws=False, stats_ld=None, k0=0, Ka=None, rows=4):
    return dict(mtiles=mtiles, K=K, ws=ws, stats_ld=stats_ld or K, k0=k0, Ka=Ka, rows=rows)


FINALIZE = {f'one-{m}': _fin(m) for m in (1, 31, 32, 33, 255, 256, 257, 600, 1024)}
FINALIZE.update({f'twostage-{m}': _fin(m, ws=True) for m in (1025, 1056, 2100)})
FINALIZE.update({f'long-{m}': _fin(m) for m in (1025, 1056, 2100)})         # no workspace: the one-stage kernel over more than 1024 slabs
FINALIZE.update({'k20': _fin(257, K=20),                                    # the last workgroup of 8 channels is half empty
                 'slice': _fin(33, stats_ld=40, k0=8),                      # channels [8, 32) of a 40-wide slab
                 'pair': _fin(257, Ka=8),                                   # two modules, the second without running statistics
                 'count1': _fin(1, rows=1), 'count2': _fin(2, rows=1)})
CONST_CH, FAR_CH, FAR_RATIO, LAST_SLAB_GAIN = 0, 1, 300.0, 8.0


@functools.lru_cache(maxsize=None)
def finalize_inputs(name):
    """slabs [mtiles][2][stats_ld]: fp32 per-tile sums of real data (POISON outside the channels [k0, k0 + K)); channel CONST_CH is
    constant (its variance cancels to <= 0), channel FAR_CH has |mean| = 300 std, every other channel's last tile is LAST_SLAB_GAIN times
    larger than the rest, so that a last slab counted twice cannot hide inside a bound."""
    c = dict(FINALIZE[name])
    mtiles, K, rows = c['mtiles'], c['K'], c['rows']
    rng = np.random.RandomState(1000 + mtiles + K)
    mu = rng.uniform(1.0, 2.0, K) * np.where(np.arange(K) % 2, -1, 1)
    sd = rng.uniform(0.1, 0.25, K)
    mu[FAR_CH] = FAR_RATIO * sd[FAR_CH]
    y = (rng.standard_normal((mtiles, rows, K)) * sd + mu).astype(F32)
    y[-1, :, 2:] *= F32(LAST_SLAB_GAIN)
    for v in (1.1, 1.3, 0.7, 0.9, 1.7, 2.3):                                # fl(v * v) > v * v for some of these: the raw variance is negative
        y[:, :, CONST_CH] = F32(v)
        s, ss = y.sum(1, dtype=F32), (y * y).sum(1, dtype=F32)
        t = s[:, CONST_CH].astype(np.float64).sum() / (mtiles * rows)
        if ss[:, CONST_CH].astype(np.float64).sum() / (mtiles * rows) - t * t < 0:
            break
    slabs = np.full((mtiles, 2, c['stats_ld']), POISON, F32)
    slabs[:, 0, c['k0']:c['k0'] + K], slabs[:, 1, c['k0']:c['k0'] + K] = s, ss
    c.update(slabs=slabs, y=y, count=mtiles * rows, gamma=(rng.uniform(0.5, 1.5, K) * np.where(np.arange(K) % 3, 1, -1)).astype(F32),
             beta=rng.uniform(-0.3, 0.3, K).astype(F32), rm=rng.uniform(-0.5, 0.5, K).astype(F32), rv=rng.uniform(0.5, 1.5, K).astype(F32))
    return c


def finalize_view(c):
    """the [mtiles][2][K] slabs the kernel is pointed at"""
    return c['slabs'][:, :, c['k0']:c['k0'] + c['K']]


# ------------------------------------------------------------------------------------------ forward
FWD_K = {'f32': (4, 48, 1028, 1072), 'bf16': (8, 48, 2056, 2144)}           # the last two: a second column chunk of 1 and of 12 vectors
FWD_M = (1, 35, 257)
FWD = [(dt, K, M) for dt in DTYPES for K in FWD_K[dt] for M in FWD_M]
ACTS = (bn_ref.ACT_NONE, bn_ref.ACT_SILU, bn_ref.ACT_RELU)
# (K, Ka): the split on the chunk boundary, off it, and in a narrow layer
PAIRS = {'f32': ((1072, 1024), (1072, 1000), (48, 16)), 'bf16': ((2144, 2048), (2144, 1000), (48, 16))}
SPECIAL = ('wide', 'zeros', 'nonfinite')
SPECIAL_M = 35


@functools.lru_cache(maxsize=None)
def coeffs(K, seed=0):
    rng = np.random.RandomState(77 + K + seed)
    scale = (rng.uniform(0.5, 1.5, K) * np.where(np.arange(K) % 5 == 2, -1, 1)).astype(F32)
    return scale, rng.uniform(-0.3, 0.3, K).astype(F32)


@functools.lru_cache(maxsize=None)
def fwd_inputs(dt, K, M, kind='plain'):
    """(y, res, scale, shift); kind 'wide': u = y * scale + shift spans [-100, 100]; 'zeros': u is exactly 0 in places (y = 0 under
    shift = 0, and y * scale = -shift exactly); 'nonfinite': NaN, +Inf and -Inf planted in y, in every column chunk"""
    rng = np.random.RandomState(K * 1000 + M + (dt == 'bf16'))
    scale, shift = (a.copy() for a in coeffs(K))
    y = rounded(rng.standard_normal((M, K)) * 1.2 + 0.3, dt)
    res = rounded(rng.uniform(-1, 1, (M, K)), dt)
    if kind == 'wide':
        scale[:], shift[:] = 1.0, 0.0
        y = rounded(np.linspace(-100, 100, M * K).reshape(K, M).T, dt)
    elif kind == 'zeros':
        scale[0::2], shift[0::2] = 1.5, 0.0
        scale[1::2], shift[1::2] = 2.0, -2.0
        y[::3, 0::2], y[1::3, 1::2] = 0.0, 1.0
    elif kind == 'nonfinite':
        cols = sorted({0, 1, 2, K // 2, K - 3, K - 2, K - 1})
        for i, k in enumerate(cols):
            y[(5 * i) % M, k] = (np.nan, np.inf, -np.inf)[i % 3]
            y[(5 * i + 2) % M, k] = (np.inf, -np.inf, np.nan)[i % 3]
    else:
        assert kind == 'plain'
    return y, res, scale, shift


# ------------------------------------------------------------------------------------------ backward
BWD_ACTS = (bn_ref.ACT_NONE, bn_ref.ACT_SILU)
BWD_WIDE = [(dt, K, M) for dt in DTYPES for K in FWD_K[dt] for M in (1, 34, 35, 65)]     # M = 65: two blocks of 33 rows
BWD_TALL = [(dt, 48, M) for dt in DTYPES for M in (150, 4000, 32769)]                     # M = 32769: 512 blocks of 65, the last seven empty
BWD_REDUCE4 = [('bf16', 1032, 65), ('bf16', 1072, 65)]                                    # the four-channel kernel's second chunk: 2 and 12 vectors
BWD_FINALIZE_WIDE = ('bf16', 8, 261889)                                                   # 1024 row blocks: bn_bwd_finalize_kernel<8, 128>
BWD = BWD_WIDE + BWD_TALL + BWD_REDUCE4 + [BWD_FINALIZE_WIDE]
BWD_PAIRS = [(dt, K, Ka, 65) for dt in DTYPES for K, Ka in PAIRS[dt]]
SLAB_COUNTS, SLAB_K = (1023, 1024, 1025, 2049), 20


@functools.lru_cache(maxsize=8)
def bwd_inputs(dt, K, M):
    """(dz, y, scale, shift, mean, invstd): the statistics are the reference's own finalize of y, rounded to fp32"""
    rng = np.random.RandomState(K * 7 + M + 13 * (dt == 'bf16'))
    y = rounded(rng.standard_normal((M, K)) * 1.2 + 0.3, dt)
    dz = rounded(rng.uniform(-1, 1, (M, K)), dt)
    gamma, beta = coeffs(K, seed=1)
    slab = np.stack([y.astype(np.float64).sum(0), (y.astype(np.float64) ** 2).sum(0)])[None]
    scale, shift, mean, invstd, _, _ = bn_ref.finalize(slab, M, gamma, beta, None, None, EPS, MOMENTUM)
    return (dz, y) + tuple(a.astype(F32) for a in (scale, shift, mean, invstd))


@functools.lru_cache(maxsize=None)
def slab_inputs(nslabs):
    """slabs [n][2][K] of (SUM du, SUM du * y) as the fused 1x1 backward's epilogue writes them, with mean / invstd"""
    rng = np.random.RandomState(nslabs)
    du = rng.uniform(-1, 1, (nslabs, 128, SLAB_K)).astype(F32)
    y = (rng.standard_normal((nslabs, 128, SLAB_K)) * 1.2 + 0.3).astype(F32)
    slabs = np.stack([du.sum(1, dtype=F32), (du * y).sum(1, dtype=F32)], 1)
    return slabs, nslabs * 128, np.full(SLAB_K, 0.3, F32) + rng.uniform(-.01, .01, SLAB_K).astype(F32), rng.uniform(0.7, 0.9, SLAB_K).astype(F32)


# ------------------------------------------------------------------------------------------ column sums, add, SyncBatchNorm, eval table
COLSUM = [(dt, K, M) for dt in DTYPES for K in (8, 1072, 2144) for M in (1, 65, 32769)]
ADD = [(dt, K, M) for dt in DTYPES for K in (FWD_K[dt][1], FWD_K[dt][3]) for M in (1, 35)]
SYNC = dict(Ktot=40, k0=8, K=24, Ka=8, nslabs=(33, 257), rows=4)
EVAL_K = (1, 8, 255, 256, 700)


def colsum_inputs(dt, K, M):
    g = torch.Generator().manual_seed(K + M)
    return (torch.rand((M, K), generator=g) * 2 - 0.5).to(TORCH[dt])


@functools.lru_cache(maxsize=None)
def sync_inputs():
    """two ranks' slab sets over Ktot channels and their element counts"""
    rng = np.random.RandomState(5)
    sets = []
    for r, n in enumerate(SYNC['nslabs']):
        y = (rng.standard_normal((n, SYNC['rows'], SYNC['Ktot'])) * (0.5 + r) + 0.4 * (r + 1)).astype(F32)
        sets.append(np.stack([y.sum(1, dtype=F32), (y * y).sum(1, dtype=F32)], 1))
    K = SYNC['K']
    return sets, [n * SYNC['rows'] for n in SYNC['nslabs']], dict(
        gamma=rng.uniform(0.5, 1.5, K).astype(F32), beta=rng.uniform(-0.3, 0.3, K).astype(F32), rm=rng.uniform(-0.5, 0.5, K).astype(F32),
        rv=rng.uniform(0.5, 1.5, K).astype(F32))


@functools.lru_cache(maxsize=None)
def eval_inputs(K, bump=0):
    rng = np.random.RandomState(K + 100 * bump)
    return dict(gamma=rng.uniform(-1.5, 1.5, K).astype(F32), beta=rng.uniform(-0.3, 0.3, K).astype(F32), rm=rng.uniform(-0.5, 0.5, K).astype(F32),
                rv=rng.uniform(0.01, 1.5, K).astype(F32))


def case_id(c):
    return '-'.join(str(v) for v in c) if isinstance(c, (tuple, list)) else str(c)


assert math.isclose(EPS, 1e-3, rel_tol=1e-6) and math.isclose(MOMENTUM, 0.03, rel_tol=1e-6)
