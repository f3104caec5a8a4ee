"""The cases of the direct tests of csrc/seg.hip, shared by test_segk_ref_host.py (which proves on the CPU that every case contains what its
name claims) and test_gpu_seg_direct.py.  Everything is generated and seeded, as exact float32 values (bf16 cases: values a bf16 holds
exactly); nothing here imports hd_yolo_amd.  Each case is the smallest tensor that reaches the named path; the launch geometry of seg.hip
(slices, row lanes, column chunks, grid caps, the backward form ops.bilinear_bwd selects, the fp32 index arithmetic of the resize) is
restated here in Python so that this can be asserted.  The largest case (gn 'cap') has 2.46 M elements.

Left out: the grid cap of dice_bwd_kernel (4096 blocks of 1024 pixels per image): reaching it needs more than 4.19 M pixels in one image.
"""
import functools

import numpy as np
import torch

import segk_ref as ref

F32 = np.float32
DTYPES = ('f32', 'bf16')
VE = {'f32': 4, 'bf16': 8}
TORCH = {'f32': torch.float32, 'bf16': torch.bfloat16}
POISON = 7.0
GN_EPS = float(F32(1e-5))
GN_SLICES, DICE_SLICES = 32, 64
GRID_CAP = 4096


def rounded(a, dt):
    """float32 array of values the arithmetic type holds exactly"""
    a = np.ascontiguousarray(a, F32)
    return torch.from_numpy(a).to(torch.bfloat16).float().numpy() if dt == 'bf16' else a


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------ GroupNorm: geometry of seg.hip, restated
def gn_geometry(N, HW, C, ve):
    """gn_reduce_kernel / gn_apply_kernel: per column chunk the vectors VC, row lanes RL and dead lanes; the set of trip counts of the live row
    lanes of the reduce over all slices; empty slices; the longest fp32 chain n = trips + RL (at most the pixels of a slice: adding a lane that holds 0 is exact); the apply grid and whether it grid-strides"""
    vct, per = C // ve, cdiv(HW, GN_SLICES)
    chunks = [min(256, vct - 256 * k) for k in range(cdiv(vct, 256))]
    out = dict(chunks=chunks, RL=[256 // vc for vc in chunks], dead=[256 - (256 // vc) * vc for vc in chunks], per=per,
               empty=sum(1 for s in range(GN_SLICES) if s * per >= HW), trips=[], n=0)
    for vc in chunks:
        RL = 256 // vc
        t = set()
        for s in range(GN_SLICES):
            cnt = max(min(s * per + per, HW) - s * per, 0)
            if cnt:
                t |= {max(cdiv(cnt - rl, RL), 0) for rl in range(RL)}
        out['trips'].append(t)
        out['n'] = max(out['n'], min(cdiv(per, RL) + RL, per))           # a sum of `per` terms has fewer roundings than that however it is ordered
    rl0 = 256 // chunks[0]
    gx = min(cdiv(HW, rl0), 2048 // min(N, 2048) + 1)
    out.update(apply_grid=gx, apply_capped=gx * rl0 < HW, apply_trips=cdiv(HW, gx * rl0))
    return out


def _gn(N, HW, C, G, kind='plain', dts=DTYPES):
    return dict(N=N, HW=HW, C=C, G=G, kind=kind, dts=dts)


GN = {
    'straddle': _gn(2, 35, 24, 4),                       # 6 channels per group: every vector straddles two groups; 4 (fp32) / 1 (bf16) dead lanes
    'g-eq-c': _gn(2, 33, 8, 8),
    'g-1': _gn(1, 5, 16, 1),                             # HW = 5: 27 empty slices
    'hw-1': _gn(3, 1, 24, 4),
    'hw-1-g-eq-c': _gn(2, 1, 8, 8, 'small'),             # one element per group: xhat = 0 and dx = k0 dy - k1 cancels to 0; rstd = eps^-1/2 = 316, so
                                                         # |x| <= 0.1 keeps the rounding of x a + b (a = 316 gamma) well below |beta|
    'trips': _gn(1, 3200, 24, 4),                        # 100 pixels per slice over 42 (fp32) / 85 (bf16) row lanes: unequal trip counts
    'chunk2-f32': _gn(2, 9, 1028, 4, dts=('f32',)),      # 257 vectors: a second column chunk of one vector and 256 row lanes
    'chunk2-bf16': _gn(2, 9, 2056, 4, dts=('bf16',)),
    'cap': _gn(8, 300, 1024, 32, dts=('f32',)),          # apply grid capped at 2048 / 8 + 1 = 257 blocks of one row lane: two trips
    'offset': _gn(2, 35, 24, 4, 'offset', ('f32',)),     # group 1: |mean| = 1000 std
    'zeros': _gn(2, 35, 24, 4, 'zeros'),                 # var == 0
    'wide': _gn(2, 35, 24, 4, 'wide'),                   # |x| up to 100
    'nan': _gn(2, 35, 24, 4, 'nan'),
    'pinf': _gn(2, 35, 24, 4, 'pinf'),
    'ninf': _gn(2, 35, 24, 4, 'ninf'),
    'nan-gamma': _gn(2, 35, 24, 4, 'nan-gamma'),
    'nan-dout': _gn(2, 35, 24, 4, 'nan-dout'),
}
GN_NONFINITE = ('nan', 'pinf', 'ninf', 'nan-gamma', 'nan-dout')
GN_CASES = [(name, dt) for name, c in GN.items() for dt in c['dts']]
BAD_AT = (1, 17, 8)                                       # (image, pixel, channel) of the planted value: group 1 of image 1


@functools.lru_cache(maxsize=None)
def gn_inputs(name, dt):
    """dict(x [N, HW, C], gamma, beta, dout, old_dg, old_db).  Neighbouring groups differ by up to 16x in scale and by several spreads in
    mean, so a statistic taken from the wrong group is far outside any bound.  Every finite pre-activation is then moved at least
    KINK_MARGIN forward bounds away from the ReLU kink (x nudged, nothing skipped), so the backward's gate is the same on both sides."""
    c = GN[name]
    N, HW, C, G, kind = (c[k] for k in ('N', 'HW', 'C', 'G', 'kind'))
    rng = np.random.RandomState(sum(map(ord, name)) * 2 + (dt == 'bf16'))
    g = np.repeat(np.arange(G), C // G)
    scale = 0.25 * 2.0 ** (g % 5)
    mean = ((g * 7) % 11 - 5) * 0.8
    x = rng.standard_normal((N, HW, C)) * scale + mean + np.arange(N)[:, None, None] * 0.5
    if kind == 'offset':
        sel = g == 1
        x[:, :, sel] = rng.standard_normal((N, HW, int(sel.sum()))) * 0.5 + 500.0
    elif kind == 'zeros':
        x[:] = 0.0
    elif kind == 'small':
        x *= 2.0 ** -6
    elif kind == 'wide':
        x = rng.uniform(-100, 100, (N, HW, C))
    x = rounded(x, dt)
    sign = np.where(np.arange(C) % 5 == 2, -1.0, 1.0)
    gamma = (rng.uniform(0.5, 1.5, C) * sign).astype(F32)
    beta = (rng.uniform(0.1, 0.4, C) * np.where(np.arange(C) % 3 == 1, -1.0, 1.0)).astype(F32)
    if kind == 'offset':                                  # rstd of this group is only guaranteed to 20 % (segk_ref): |beta| >> |gamma xhat| keeps the kink away
        gamma[g == 1] *= F32(2.0 ** -5)
        beta[g == 1] *= F32(8)
    dout = rounded(rng.uniform(-1, 1, (N, HW, C)), dt)
    n = gn_geometry(N, HW, C, VE[dt])['n']
    for it in range(60):
        _, pre = ref.gn_forward(x, gamma, beta, G, GN_EPS, True)
        bound = ref.gn_forward_bound(x, gamma, beta, G, GN_EPS, n)
        off = np.abs(pre) < 1.5 * ref.KINK_MARGIN * bound
        if not off.any() or kind in ('zeros', 'small'):
            break
        _, var = ref.gn_stats(x, G)
        a = np.abs(np.repeat(1.0 / np.sqrt(var + GN_EPS), C // G, 1)[:, None, :] * gamma)
        x = rounded(np.where(off, x + 0.1 * (it + 1) / a, x), dt)
    else:
        raise AssertionError(f'{name} {dt}: pre-activations still at the kink')
    bn, bp, bc_ = BAD_AT
    if kind in ('nan', 'pinf', 'ninf'):
        x[bn, min(bp, HW - 1), bc_] = {'nan': np.nan, 'pinf': np.inf, 'ninf': -np.inf}[kind]
    elif kind == 'nan-gamma':
        gamma[bc_] = np.nan
    elif kind == 'nan-dout':
        dout[bn, min(bp, HW - 1), bc_] = np.nan
    return dict(x=x, gamma=gamma, beta=beta, dout=dout, old_dg=np.linspace(-2, 2, C).astype(F32), old_db=np.linspace(3, -1, C).astype(F32))


# ------------------------------------------------------------------------------------------ resize
def scale32(n_in, n_out):
    return F32(n_in - 1) / F32(n_out - 1) if n_out > 1 else F32(0)


@functools.lru_cache(maxsize=None)
def index32(n_in, n_out):
    """src_index of seg.hip in float32 for every output index: arrays (i0, i1, l0, l1)"""
    s = (scale32(n_in, n_out) * np.arange(n_out, dtype=F32)).astype(F32)
    a = np.minimum(s.astype(np.int64), n_in - 1)
    l1 = (s - a.astype(F32)).astype(F32)
    return a, a + (a < n_in - 1), (F32(1) - l1).astype(F32), l1


def dst_range32(i, n_in, n_out, margin=1):
    """dst_range of seg.hip in float32; margin=0: the range without its safety margin"""
    sc = scale32(n_in, n_out)
    if sc <= 0:
        return 0, n_out - 1
    a = int(np.floor((F32(i) - F32(1)) / sc)) - margin
    b = int(np.ceil((F32(i) + F32(1)) / sc)) + margin
    return max(a, 0), min(b, n_out - 1)


def contributors32(i, n_in, n_out):
    """outputs whose fp32 src_index touches input i with a nonzero weight"""
    i0, i1, l0, l1 = index32(n_in, n_out)
    return np.nonzero(np.where(i0 == i, l0, 0) + np.where(i1 == i, l1, 0))[0]


def bwd_form(in_size, out_size):
    """what ops.bilinear_bwd runs: the W pass and the H pass where both axes grow at least twofold, else the 2-D gather"""
    return 'two-pass' if out_size[1] >= 2 * in_size[1] and out_size[0] >= 2 * in_size[0] else '2d'


def w_pass_kernel(Ao, C, ve, inner=1):
    """hdy_bilinear_bwd_axis: the LDS kernel for inner == 1 and a gradient row of at most 64 KB"""
    return 'lds' if inner == 1 and Ao * (C // ve) * 16 <= 64 * 1024 else 'global'


RESIZE = {                                                # name: (N, input size, output size)
    'x2': (2, (5, 7), (10, 14)),
    'x8': (2, (8, 12), (64, 96)),
    'identity': (2, (6, 5), (6, 5)),
    'mixed': (2, (9, 4), (5, 11)),                        # H shrinks, W grows: the 2-D gather
    'h-in-1': (2, (1, 6), (3, 6)),
    'w-in-1': (2, (6, 1), (6, 5)),
    'h-out-1': (2, (4, 5), (1, 10)),
    'w-out-1': (2, (4, 5), (8, 1)),
    'down': (2, (16, 16), (8, 8)),                        # inputs 1 and 14 of each axis receive nothing
    'wide-ratio-2d': (2, (4, 3), (7, 40)),                # the 2-D gather at W ratio 13
    'long-row': (2, (3, 300), (5, 2400)),                 # with three vectors the gradient row is 115 KB: beyond the LDS stage
    'flip': (2, (3, 4), (42, 22)),                        # fp32 scale * dst lands below an integer the exact product reaches (H), above in - 1 (W)
    'rows-4100': (1, (2, 2), (4100, 4)),                  # more than 4096 rows: forward, W pass (4100 rows) and H pass
}
RESIZE_VECTORS = (1, 3)
RESIZE_CASES = [(name, dt, nv) for name in RESIZE for dt in DTYPES for nv in RESIZE_VECTORS]
LDS_EDGE = dict(Ao=1366, Ai=171, nv=3, rows=3)            # 1366 x 3 vectors x 16 B = 65568 B: 32 B over the LDS limit; one vector: 21856 B


@functools.lru_cache(maxsize=8)
def resize_inputs(name, dt, nv):
    """dict(x [N, Hi, Wi, C], base (what the output holds under accumulate), dy [N, Ho, Wo, C], dbase)"""
    N, (Hi, Wi), (Ho, Wo) = RESIZE[name]
    C = nv * VE[dt]
    rng = np.random.RandomState(sum(map(ord, name)) + nv + 10 * (dt == 'bf16'))
    u = lambda *s: rounded(rng.uniform(-1, 1, s) * (1 + 3 * rng.uniform(0, 1, (1, 1, 1, s[-1]))), dt)          # noqa: E731
    return dict(x=u(N, Hi, Wi, C), base=u(N, Ho, Wo, C), dy=u(N, Ho, Wo, C), dbase=u(N, Hi, Wi, C))


# ------------------------------------------------------------------------------------------ soft dice
def dice_geometry(HW, nc, ld):
    """MAXC of the kernel template, the 16-byte pixel path, pixels in flight, the fp32 chain of a slice sum (a lane's pixels, 6 shuffle steps,
    4 waves) and whether a thread's last batch of four is clamped"""
    maxc = 4 if nc <= 4 else 8 if nc <= 8 else 32
    U_ = 4 if maxc <= 8 else 1
    per = cdiv(HW, DICE_SLICES)
    clamp = False
    for s in range(DICE_SLICES):
        p0, p1 = s * per, min(s * per + per, HW)
        for t in range(256):
            for pb in range(p0 + t, p1, 256 * U_):
                clamp |= any(pb + 256 * u >= p1 for u in range(1, U_))
    return dict(maxc=maxc, vector=maxc == 4 and ld % 4 == 0, U=U_, n=cdiv(per, 256) + 10, tail_clamp=clamp, bwd_blocks=min(max(cdiv(HW, 1024), 1), 4096))


def _dice(N, H, W, nc, ld, weights=False, upstream=None, spread=12.0, kind='plain'):
    return dict(N=N, H=H, W=W, nc=nc, ld=ld, weights=weights, upstream=upstream, spread=spread, kind=kind)


DICE = {f'nc{nc}-ld4': _dice(2, 37, 29, nc, 4, weights=nc == 3, upstream=1.7 if nc % 2 else None) for nc in (1, 2, 3, 4)}
DICE.update({
    'nc3-ld8': _dice(2, 37, 29, 3, 8, upstream=0.6),                      # 8 & 3 == 0: still the 16-byte path, channel 3 zeroed, 4..7 untouched
    'nc3-ld6': _dice(2, 37, 29, 3, 6, weights=True, upstream=0.6),        # a pitch that is no multiple of 4: the scalar loads and stores of the
    'nc1-ld5': _dice(2, 37, 29, 1, 5),                                    # MAXC == 4 kernels, the padding gradient is not written
    'nc2-ld7': _dice(2, 37, 29, 2, 7, upstream=-1.3),
    'nc4-ld5': _dice(2, 37, 29, 4, 5, weights=True),
    'nc2-ld12': _dice(2, 37, 29, 2, 12, weights=True),                    # the 16-byte path at a wider pitch
    'nc5': _dice(2, 37, 29, 5, 8, weights=True, upstream=1.7), 'nc5-plain': _dice(2, 37, 29, 5, 12),
    'nc8': _dice(2, 37, 29, 8, 8, upstream=-2.5), 'nc8-w': _dice(2, 37, 29, 8, 12, weights=True),
    'nc9': _dice(2, 37, 29, 9, 12, weights=True, upstream=1.7), 'nc9-plain': _dice(2, 37, 29, 9, 9),
    'nc32': _dice(2, 37, 29, 32, 40, upstream=0.3), 'nc32-w': _dice(2, 37, 29, 32, 32, weights=True),
    'hw1': _dice(3, 1, 1, 3, 4), 'hw63': _dice(2, 7, 9, 3, 4, upstream=1.7), 'hw65': _dice(2, 5, 13, 3, 4, weights=True),
    'hw1025': _dice(2, 25, 41, 3, 4),
    'spread80': _dice(2, 37, 29, 3, 4, spread=80.0, upstream=1.7),        # probabilities that underflow: the absolute floor
    'empty-class': _dice(2, 37, 29, 3, 4, kind='empty-class'),            # all-zero targets for class 1: prod = 0 exactly
    'nan': _dice(3, 37, 29, 3, 4, kind='nan', upstream=1.7),
})
DICE_NAN_AT = (1, 500, 2)                                 # (image, pixel, class)
WGRAD = {'w40': (2, 5, 40, 3, 5), 'w64-nc1': (2, 3, 64, 1, 8), 'rows-4098': (2, 2049, 8, 4, 2)}          # (N, H, W, nc, Wi); the last: N H > 4096
SOFTMAX2D = ((1, 4), (3, 8), (8, 12))                     # (nc, pitch of the logits)


@functools.lru_cache(maxsize=None)
def dice_inputs(name):
    """dict(logits [N, HW, ld] with POISON-like garbage in the padding channels, targets [N, nc, HW] one-hot, weights or None)"""
    c = DICE[name] if name in DICE else _dice(*WGRAD[name][:4], 4, weights=WGRAD[name][3] == 3)
    N, HW, nc, ld = c['N'], c['H'] * c['W'], c['nc'], c['ld']
    rng = np.random.RandomState(sum(map(ord, name)))
    logits = rng.uniform(-c['spread'], c['spread'], (N, HW, ld)).astype(F32)
    logits[..., nc:] = rng.uniform(50, 90, (N, HW, ld - nc)).astype(F32)                # garbage that would win the max
    lab = rng.randint(0, max(nc, 2), (N, HW))
    if c['kind'] == 'empty-class':
        lab[lab == 1] = 0
    targets = np.stack([(lab == k).astype(F32) for k in range(nc)], 1)
    if c['kind'] == 'nan':
        logits[DICE_NAN_AT] = np.nan
    weights = rng.uniform(0.5, 2.0, nc).astype(F32) if c['weights'] else None
    return dict(c, HW=HW, logits=logits, targets=targets, cw=weights)


def case_id(c):
    return '-'.join(str(v) for v in c) if isinstance(c, (tuple, list)) else str(c)
