"""Named inputs for the direct tests of csrc/roi.hip (tests/test_gpu_roi_direct.py); tests/test_roi_ref_host.py proves on the CPU what each
contains.  Plain numpy, seeded; the kernel's launch decisions (footprint, tiled or scatter path) are restated here in fp32 from
roi_ref.geometry(..., np.float32), and the constants FT / PM / CB below are compared with the text of roi.hip by the host test.

A roi set is built from classes, each placed by its first and last sample coordinate in feature pixels (`axis_for`), so what a class is
named for holds for every P, S and `aligned`:
    overlap   8 rois a few pixels wide that all cover one feature pixel         narrow   0.4 pixels wide; zero: x1 == x2, y1 == y2
    interior  a few pixels wide, images 0 and 2                                 left / right / top / bottom: samples in [-1, 0) or (size - 1, size],
    outside   every sample of one axis beyond the thresholds                              and beyond the thresholds where P S allows
    img-1 / imgB  image index -1 and B                                         whole    the whole map
    fp24x24, fp24x25, fp25x24, fp30x30   footprints of exactly that many rows x columns, extreme samples 0.3 / 0.4 away from an integer
Image 1 of 3 is named by no roi.  Sets: 'small' (footprints <= FT: the tiled path when P <= PM), 'large' (> FT: the scatter path), 'mixed'.
"""
import numpy as np

import roi_ref

FT, PM, CB = 24, 16, 32                       # roi.hip: footprint tile side, largest tiled P, channels per workgroup
VE = {'f32': 4, 'bf16': 8}
DTYPES = ('f32', 'bf16')
POISON = 7.0
B = 3
UNNAMED = 1                                   # the image no roi names


def q(a, dt):
    """round to the tensor type's values (bf16: round to nearest even on the upper 16 bits), returned as float32"""
    a = np.ascontiguousarray(a, np.float32)
    if dt == 'f32':
        return a
    u = a.view(np.uint32).astype(np.uint64)
    u = ((u + 0x7fff + ((u >> 16) & 1)) >> 16) << 16
    out = u.astype(np.uint32).view(np.float32)
    return np.where(np.isfinite(a), out, a)


# ------------------------------------------------------------------------------------------ the kernel's decisions, in fp32
def closed_form_footprint(g, P, S, H, W):
    """the footprint rule roi.hip had before it took the footprint from the samples: y0 + (P - 0.5 / S) bin for the top sample, fp32
    operation for operation -> (fy0, fy1, fx0, fx1)"""
    f = np.float32
    out = []
    with np.errstate(all='ignore'):
        for o, bs, size in ((g['y0'], g['bin_h'], H), (g['x0'], g['bin_w'], W)):
            lo = (o + ((f(0.5) * bs).astype(f) / f(S)).astype(f)).astype(f)
            hi = (o + ((f(P) - f(0.5) / f(S)).astype(f) * bs).astype(f)).astype(f)
            fl = lambda v: np.floor(np.maximum(np.where(np.isnan(v), f(0), v), f(0))).astype(np.int64)         # noqa: E731
            out += [np.clip(fl(lo), 0, size - 1), np.clip(fl(hi) + 1, 0, size - 1)]
    return tuple(out)


def classify(rois, scale, P, S, aligned, nb, H, W, rule='samples'):
    """what roi_align_bwd_tiled_kernel decides per roi, in fp32: live (image in [0, nb) and a valid sample on both axes), the index range
    [lo, hi] of the valid samples per axis, the footprint by `rule` ('samples': that range, the kernel's rule; 'closed': the closed form),
    tiled, and escape: a valid sample index outside the footprint (a table write past its row)"""
    g = roi_ref.geometry(rois, scale, P, S, aligned, np.float32)
    R = len(g['b'])
    rng = {}
    for ax, size in (('y', H), ('x', W)):
        ok, i0, i1, _, _ = roi_ref.axis_sample(g[ax + 's'], size)
        big = np.iinfo(np.int64).max
        rng[ax] = (np.where(ok, i0, big).min(1) if R else np.zeros(0, np.int64), np.where(ok, i1, -1).max(1) if R else np.zeros(0, np.int64), ok.any(1))
    live = (g['b'] >= 0) & (g['b'] < nb) & rng['y'][2] & rng['x'][2]
    if rule == 'samples':
        fy0, fy1, fx0, fx1 = rng['y'][0], rng['y'][1], rng['x'][0], rng['x'][1]
    else:
        fy0, fy1, fx0, fx1 = closed_form_footprint(g, P, S, H, W)
    fh, fw = fy1 - fy0 + 1, fx1 - fx0 + 1
    esc_y = rng['y'][2] & ((rng['y'][0] < fy0) | (rng['y'][1] > fy1))
    esc_x = rng['x'][2] & ((rng['x'][0] < fx0) | (rng['x'][1] > fx1))
    return dict(live=live, fh=np.where(live, fh, 0), fw=np.where(live, fw, 0), fy0=fy0, fy1=fy1, fx0=fx0, fx1=fx1,
                tiled=live & (fh <= FT) & (fw <= FT) & (P <= PM), scatter=live & ~((fh <= FT) & (fw <= FT) & (P <= PM)),
                escape_y=esc_y & (g['b'] >= 0) & (g['b'] < nb), escape_x=esc_x & (g['b'] >= 0) & (g['b'] < nb), geom=g)


# ------------------------------------------------------------------------------------------ roi sets
def axis_for(first, last, P, S, aligned, scale, single='first'):
    """(c1, c2) roi coordinates of one axis whose first sample lies at `first` and whose last at `last` (feature pixels)"""
    off = 0.5 if aligned else 0.0
    if P * S == 1:
        bs = 1.0
        o = (last if single == 'last' else first) - 0.5
    else:
        bs = (last - first) / (P - 1.0 / S)
        o = first - bs / (2 * S)
    return (o + off) / scale, (o + P * bs + off) / scale


def build_set(kind, P, S, aligned, scale, H, W, seed=0):
    """-> (rois [R, 5] fp32, classes [R])"""
    rng = np.random.RandomState(1000 + seed)
    rois, cls = [], []

    def add(name, img, xf, xl, yf, yl, single='first'):
        x1, x2 = axis_for(xf, xl, P, S, aligned, scale, single)
        y1, y2 = axis_for(yf, yl, P, S, aligned, scale, single)
        rois.append([img, x1, y1, x2, y2])
        cls.append(name)

    if kind in ('small', 'mixed'):
        for k in range(8):
            add('overlap', 0, 19.2 + 0.09 * k, 22.4 + 0.13 * k, 19.3 + 0.08 * k, 21.3 + 0.11 * k)
        for k in range(6):
            xf, yf = rng.uniform(2, W - 12), rng.uniform(2, H - 12)
            add('interior', 0 if k % 2 else 2, xf, xf + rng.uniform(1.5, 9), yf, yf + rng.uniform(1.5, 9))
        off = 0.5 if aligned else 0.0
        rois.append([2, (10.3 + off) / scale, (12.2 + off) / scale, (10.7 + off) / scale, (12.6 + off) / scale])
        cls.append('narrow')
        rois.append([0, (30.3 + off) / scale, (7.4 + off) / scale, (30.3 + off) / scale, (7.4 + off) / scale])
        cls.append('zero')
        add('left', 0, -0.6, 3.3, 5.3, 9.4)
        add('right', 2, W - 2.6, W - 0.4, 25.3, 29.4, 'last')
        add('top', 2, 20.3, 25.4, -0.7, 2.3)
        add('bottom', 0, 33.3, 38.4, H - 3.7, H - 0.3, 'last')
        add('left', 2, -2.6, 4.3, 15.3, 19.4)                         # and with samples beyond -1 / size (where P S > 1)
        add('bottom', 2, 3.3, 8.4, H - 4.7, H + 1.6, 'last')
        add('outside', 0, W + 1.5, W + 4.5, 5.3, 9.4)
        add('outside', 2, 5.3, 9.4, -5.5, -1.6)
        add('img-1', -1, 6.3, 11.4, 6.3, 11.4)
        add('imgB', B, 6.3, 11.4, 6.3, 11.4)
    if kind == 'mixed':
        add('fp24x24', 0, 10.3, 32.4, 8.3, 30.4)
    if kind in ('large', 'mixed'):
        rois.append([0, 0.0, 0.0, W / scale, H / scale])
        cls.append('whole')
        add('fp30x30', 2, 5.3, 33.4, 4.3, 32.4)
        add('fp24x25', 0, 12.3, 35.4, 9.3, 31.4)                     # 24 rows, 25 columns
        add('fp25x24', 2, 11.3, 33.4, 6.3, 29.4)
        add('left', 0, -0.7, 30.3, 2.3, 33.4)
    return np.array(rois, np.float32), cls


FP_CLASSES = {'fp24x24': (24, 24), 'fp24x25': (24, 25), 'fp25x24': (25, 24), 'fp30x30': (30, 30)}
H, W = 40, 48

# (P, S, aligned, set, index into the dtype's channel counts, scale): every P with both dtypes; P <= PM with the tiled and the scatter path
_GRID = [(14, 2, False, 'small', 0, 0.125), (14, 2, True, 'large', 1, 0.125), (14, 2, False, 'mixed', 2, 0.0625), (7, 1, True, 'small', 1, 0.125),
         (7, 3, False, 'large', 0, 0.0625), (7, 4, True, 'mixed', 2, 0.125), (16, 2, True, 'small', 2, 0.0625), (16, 4, False, 'large', 1, 0.125),
         (16, 3, False, 'mixed', 0, 0.125), (1, 1, False, 'small', 0, 0.125), (1, 4, True, 'large', 1, 0.0625), (1, 2, True, 'mixed', 2, 0.125),
         (17, 2, False, 'small', 1, 0.125), (17, 1, True, 'mixed', 0, 0.0625), (28, 2, True, 'small', 2, 0.125), (28, 3, False, 'large', 0, 0.125),
         (14, 1, True, 'mixed', 1, 0.125), (14, 3, True, 'small', 0, 0.0625), (14, 4, False, 'large', 2, 0.125), (16, 1, False, 'mixed', 1, 0.0625)]
CHANNELS = {'f32': (4, 36, 72), 'bf16': (8, 40, 72)}
GRID = [(dt, CHANNELS[dt][ci], P, S, al, kind, sc) for dt in DTYPES for P, S, al, kind, ci, sc in _GRID]


def case_id(c):
    return '-'.join('aligned' if v is True else 'legacy' if v is False else str(v) for v in c)


def _features(seed, shape, dt):
    rng = np.random.RandomState(seed)
    return q(rng.standard_normal(shape), dt)


def make(dt, C, P, S, aligned, rois, nb, h, w, scale, seed=0, cls=None):
    feat = _features(11 + seed, (nb, h, w, C), dt)
    dout = _features(23 + seed, (len(rois), P, P, C), dt)
    into = np.random.RandomState(5 + seed).standard_normal((nb, h, w, C)).astype(np.float32)
    return dict(dt=dt, C=C, P=P, S=S, aligned=aligned, scale=scale, B=nb, H=h, W=w, rois=np.asarray(rois, np.float32), cls=cls or ['-'] * len(rois),
                feat=feat, dout=dout, into=into)


def grid_case(c):
    dt, C, P, S, aligned, kind, scale = c
    rois, cls = build_set(kind, P, S, aligned, scale, H, W, seed=P * 10 + S)
    return make(dt, C, P, S, aligned, rois, B, H, W, scale, seed=P + S, cls=cls)


# H == 1 and W == 1 maps, and the dyadic threshold case (samples exactly on -1 and on size: every coordinate is a multiple of 1/8)
SPECIAL = ['h1', 'w1', 'dyadic']


def special_case(name, dt):
    C = {'f32': 4, 'bf16': 8}[dt]
    if name == 'dyadic':
        rois = [[0, -18, -18, 110, 110], [1, -10, -18, 118, 110], [0, -18, 6, 110, 70]]
        return make(dt, C, 16, 2, False, rois, 2, 13, 13, 0.125, seed=3)
    P, S, scale = 7, 2, 0.125
    h, w = (1, 20) if name == 'h1' else (20, 1)
    rois = []
    for aligned_like, (f, l) in enumerate(((-0.6, 0.6), (-0.3, 0.4), (-2.6, 1.7))):           # the one-pixel axis: inside [-1, 1] and beyond both
        a1, a2 = axis_for(f, l, P, S, False, scale)
        b1, b2 = axis_for(3.3 + aligned_like, 9.4 + 2 * aligned_like, P, S, False, scale)
        rois.append([aligned_like % 2, b1, a1, b2, a2] if name == 'h1' else [aligned_like % 2, a1, b1, a2, b2])
    return make(dt, C, P, S, False, rois, 2, h, w, scale, seed=4)


def plant_nonfinite_features(c):
    """dyadic case: a NaN and an infinity in image 0"""
    f = c['feat'].copy()
    f[0, 5, 5, 1] = np.nan
    f[0, 9, 3, 2] = np.inf
    return f


NONFINITE_BWD = [('f32', 36, 14, 2, False, 'mixed', 0.125), ('bf16', 40, 14, 2, False, 'mixed', 0.125)]
NONFINITE_AT = (('interior', (3, 4), 1, np.nan), ('fp30x30', (5, 6), 2, np.inf))          # class (its first roi), bin, channel, value


def plant_nonfinite_dout(c):
    d = c['dout'].copy()
    which = np.zeros((len(c['rois']), c['C']), bool)
    for name, (p, qq), ch, val in NONFINITE_AT:
        r = c['cls'].index(name)
        d[r, p, qq, ch] = val
        which[r, ch] = True
    return d, which


# ------------------------------------------------------------------------------------------ the closed-form footprint's misses
# Rois whose top sample index lies outside the closed-form footprint in fp32 (found by `search_misses`, seeded; the host test re-derives the
# property): (name, P, S, aligned, scale, H, W, roi).  The '24' ones have a closed-form footprint of exactly FT on the named axis at P = PM,
# so the stray write of table row PM - 1 is the first entry of the next array (the last Wy row runs into Wx[0], the last Wx row into D[0]).
MISSES = [
    ('y-legacy', 14, 2, False, 0.125, 48, 48, [0.0, 64.0, 95.8994369506836, 160.0, 275.2018127441406]),
    ('x-legacy', 14, 2, False, 0.125, 48, 48, [0.0, 95.8994369506836, 64.0, 275.2018127441406, 160.0]),
    ('y-aligned', 14, 2, True, 0.125, 48, 48, [0.0, 64.0, 96.59117889404297, 160.0, 279.261962890625]),
    ('x-aligned', 14, 2, True, 0.125, 48, 48, [0.0, 96.59117889404297, 64.0, 279.261962890625, 160.0]),
    ('wy-last-24', 16, 2, False, 0.125, 48, 48, [0.0, 64.0, 20.816299438476562, 160.0, 202.84417724609375]),
    ('wx-last-24', 16, 2, False, 0.125, 48, 48, [0.0, 20.816299438476562, 64.0, 202.84417724609375, 160.0]),
    ('wy-last-24-aligned', 16, 2, True, 0.125, 48, 48, [0.0, 64.0, 20.816299438476562, 160.0, 206.9076690673828]),
]
MISS_SEARCH = {'y-legacy': ('y', None), 'x-legacy': ('x', None), 'y-aligned': ('y', None), 'x-aligned': ('x', None), 'wy-last-24': ('y', FT),
               'wx-last-24': ('x', FT), 'wy-last-24-aligned': ('y', FT)}        # search_misses(P, S, aligned, scale, H, W, axis, 0, want_n) found each


def search_misses(P, S, aligned, scale, H, W, axis, seed, want_n=None, tries=4000, span=96):
    """rois of a scale^-1 * (W, H) tile whose last sample on `axis` has i1 beyond the closed-form footprint: random corners, the far corner
    swept `span` fp32 values either side of where the closed-form upper end meets an integer.  want_n: closed-form footprint size on the axis."""
    rng = np.random.RandomState(seed)
    f = np.float32
    size = H if axis == 'y' else W
    off = 0.5 if aligned else 0.0
    found = []
    lo = rng.uniform(0, (size - 26) / scale, tries).astype(f)
    o = lo.astype(np.float64) * scale - off
    k = np.floor(np.maximum(o, 0)) + (want_n - 1 if want_n else rng.randint(3, 24, tries))
    hi0 = ((k - o) / (P - 0.5 / S) * P + o + off) / scale
    hi = hi0.astype(f)[:, None]
    for _ in range(span):
        hi = np.concatenate([np.nextafter(hi[:, :1], f(-np.inf)), hi, np.nextafter(hi[:, -1:], f(np.inf))], 1)
    other = (f(8.0 / scale), f(20.0 / scale))
    n = hi.shape[1]
    rois = np.zeros((tries * n, 5), f)
    a, b = ((2, 4), (1, 3)) if axis == 'y' else ((1, 3), (2, 4))
    rois[:, a[0]], rois[:, a[1]] = np.repeat(lo, n), hi.reshape(-1)
    rois[:, b[0]], rois[:, b[1]] = other
    c = classify(rois, scale, P, S, aligned, 1, H, W, rule='closed')
    hit = c['escape_' + axis] & ((c['fh' if axis == 'y' else 'fw'] == want_n) if want_n else True)
    return rois[hit]


def miss_case(m, dt='f32'):
    name, P, S, aligned, scale, h, w, roi = m
    near = [roi[0], roi[1] + 5.3, roi[2] + 6.1, roi[3] - 3.3, roi[4] - 2.7]                  # an ordinary roi that overlaps it
    return make(dt, 36 if dt == 'f32' else 40, P, S, aligned, [roi, near], 1, h, w, scale, seed=9)


# ------------------------------------------------------------------------------------------ multi-level
LEVEL_SIDES, LEVEL_SCALES, MAX_DET = (4, 2), (0.25, 0.125), 3               # a 16 x 16 tile
LEVELS = [(1, 7), (4, 7), (5, 7), (260, 2), (1024, 2)]                      # (images, P)
_KEEP = (2, 0, -2, 5, 3, 1)                                                 # zeros, negative values, values above MAX_DET


def levels_case(nb, P, dt):
    rng = np.random.RandomState(nb)
    C = VE[dt]
    feats = [_features(31 + l, (nb, s, s, C), dt) for l, s in enumerate(LEVEL_SIDES)]
    n_keep = np.array([_KEEP[b % len(_KEEP)] for b in range(nb)], np.int32)
    xy = rng.uniform(-3, 12, (nb, MAX_DET, 2))
    boxes = np.concatenate([xy, xy + rng.uniform(0.5, 9, (nb, MAX_DET, 2))], 2).astype(np.float32)
    for _ in range(20):                                                     # redraw a box with a sample near a validity threshold of either level
        flat = np.concatenate([np.zeros((nb * MAX_DET, 1), np.float32), boxes.reshape(-1, 4)], 1)
        near = np.minimum(*(roi_ref.kink_distance(flat, sc, P, 2, False, s, s, per_roi=True) for s, sc in zip(LEVEL_SIDES, LEVEL_SCALES))) < 4 * roi_ref.KINK_MARGIN
        if not near.any():
            break
        xy = rng.uniform(-3, 12, (int(near.sum()), 2))
        boxes.reshape(-1, 4)[near] = np.concatenate([xy, xy + rng.uniform(0.5, 9, xy.shape)], 1).astype(np.float32)
    level = rng.randint(0, 2, (nb, MAX_DET)).astype(np.float32)
    odd = (7.0, np.nan, -0.5, np.inf, -1.0, 2.0)                            # -0.5 truncates to level 0; the others name no level
    for b in range(0, nb, 3):
        level[b, b % MAX_DET] = odd[(b // 3) % len(odd)]
    return dict(dt=dt, C=C, P=P, S=2, B=nb, feats=feats, scales=LEVEL_SCALES, boxes=boxes, level=level, n_keep=n_keep)
