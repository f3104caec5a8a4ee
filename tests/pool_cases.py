"""Named inputs for the direct tests of csrc/pool.hip (tests/test_gpu_pool_direct.py); tests/test_pool_ref_host.py proves on the CPU what each
contains and that the selection rules below are those of the launchers' text.  Plain numpy, seeded.

Selection.  `fwd_variant` / `bwd_variant` restate hdy_sppf_pool_fwd / hdy_sppf_pool_bwd: a variant is taken when its channel group divides C
and its planes fit LDS bytes, pix = (H + 4)(W + 4) padded pixels, per pixel and channel 2 plane elements plus the position bytes.  `LIMIT`
holds the largest pix per variant, recomputed here from those expressions; every boundary case below sits on one (asserted by the host test).
The names are the ones the launchers write to the dispatch log.

SPPF input families (`family`): random; ties (a grid of 1/1.5) and a constant plane; +0 / -0 mixed with -0-only windows at every level; one
NaN, several NaNs in one window, NaNs in the corners, a NaN-only plane; +inf; -inf: whole planes, the first two rows and columns, everything
but one value.  Layouts: 'plan' (x, y1, y2, y3 are the four channel slices of one [N, H, W, 4C] buffer) and 'wide' (the same buffer with 8
more channels of 7.0 on either side); position tables always sit inside a larger byte buffer.  Every pointer is 16-byte aligned; misaligned
pointers are not driven.

The 64-bit index variants of the upsample and stem_prep kernels need 2^31 vectors (32 GB and more) and are left out.  The cases above the
grid cap of 4096 x 256 threads are the smallest two-dimensional planes at a channel count the model has: one forward, one backward, one
stem_prep.
"""
import numpy as np

from pool_ref import q

LDS, PB, CG = 150 * 1024, 2, 8               # pool.hip: dynamic LDS granted to the SPPF kernels, border pixels, narrowest channel group
GRID_CAP = 4096 * 256                         # sgrid(): threads of the largest grid the elementwise kernels are launched with
DTYPES = ('f32', 'bf16')
VE = {'f32': 4, 'bf16': 8}
POISON = 7.0


def pix(H, W):
    return (H + 2 * PB) * (W + 2 * PB)


# ------------------------------------------------------------------------------------------ the launchers' rules
def _fits(H, W, cg, elem, pos_planes):
    return pix(H, W) * cg * (2 * elem + pos_planes) <= LDS


def fwd_variant(dt, H, W, C, positions, no_keys=False):
    """the name hdy_sppf_pool_fwd logs, or None where it refuses"""
    assert C % CG == 0
    ix = 1 if positions else 0
    sfx = '_pos' if positions else ''
    if dt == 'bf16':
        for keys in ((True, False) if not no_keys else (False,)):
            for cg in (32, 16):
                if C % cg == 0 and _fits(H, W, cg, 2, ix):
                    return f'sppf_fwd_{"keys" if keys else "float"}{cg}{sfx}'
    return f'sppf_fwd_c8{sfx}' if _fits(H, W, CG, 4, ix) else None


def bwd_variant(dt, H, W, C):
    assert C % CG == 0
    if dt == 'bf16' and C % 16 == 0 and _fits(H, W, 16, 4, 2):
        return 'sppf_bwd_c16'
    if _fits(H, W, CG, 4, 2):
        return 'sppf_bwd_c8_two'
    return 'sppf_bwd_c8_one' if _fits(H, W, CG, 4, 1) else None


def _limit(cg, elem, pos_planes):
    return LDS // (cg * (2 * elem + pos_planes))


LIMIT = {'fwd32_pos': _limit(32, 2, 1), 'fwd16_pos': _limit(16, 2, 1), 'fwd8_pos': _limit(CG, 4, 1),
         'fwd32': _limit(32, 2, 0), 'fwd16': _limit(16, 2, 0), 'fwd8': _limit(CG, 4, 0),
         'bwd16': _limit(16, 4, 2), 'bwd8_two': _limit(CG, 4, 2), 'bwd8_one': _limit(CG, 4, 1)}
FWD_NAMES = [f'sppf_fwd_{v}{s}' for v in ('keys32', 'keys16', 'float32', 'float16', 'c8') for s in ('_pos', '')]
BWD_NAMES = ['sppf_bwd_c16', 'sppf_bwd_c8_two', 'sppf_bwd_c8_one']
NAN_POLICY = {n: ('first' if 'keys' in n else 'last') for n in FWD_NAMES}


# ------------------------------------------------------------------------------------------ SPPF cases
# training form (with positions; the test also runs the inference form on each): (N, H, W, C) -> what the shape is there for
TRAIN = {
    'bf16': [((1, 1, 1, 32), 'keys32'), ((1, 20, 20, 32), 'keys32'), ((2, 5, 7, 64), 'keys32: two groups, two images'),
             ((1, 20, 36, 32), 'keys32 at fwd32_pos; bwd16 at its limit'), ((1, 27, 27, 32), 'keys16 one past fwd32_pos; bwd8_two one past bwd16'),
             ((2, 6, 5, 48), 'keys16: C no multiple of 32'), ((3, 4, 9, 16), 'keys16'), ((1, 36, 44, 16), 'keys16 at fwd16_pos; bwd8_two at its limit'),
             ((1, 40, 40, 16), 'c8 past fwd16_pos; bwd8_one past bwd8_two'), ((2, 6, 6, 8), 'c8'), ((1, 9, 4, 24), 'c8'), ((1, 42, 42, 8), 'c8'),
             ((1, 23, 75, 8), 'c8 at fwd8_pos; bwd8_one at its limit'), ((1, 5, 7, 8), 'c8')],
    'f32': [((1, 1, 1, 8), 'c8'), ((2, 1, 9, 8), 'c8: one row'), ((1, 9, 1, 16), 'c8: one column'), ((1, 5, 7, 8), 'c8'), ((1, 20, 20, 8), 'c8'),
            ((1, 40, 40, 8), 'c8; bwd8_one'), ((3, 6, 5, 24), 'c8'), ((1, 23, 75, 8), 'c8 at fwd8_pos; bwd8_one at its limit'),
            ((1, 20, 36, 16), 'bwd8_two below bwd16'), ((1, 27, 27, 16), 'bwd8_two'), ((1, 36, 44, 16), 'bwd8_two at its limit')],
}
# inference form only (their planes do not fit the training form's variant, or not at all)
INFER = {
    'bf16': [((1, 30, 30, 32), 'keys32'), ((1, 26, 36, 32), 'keys32 at fwd32'), ((1, 31, 31, 32), 'keys16 past fwd32'),
             ((1, 44, 46, 16), 'keys16 at fwd16'), ((1, 44, 46, 8), 'c8 at fwd8')],
    'f32': [((1, 45, 44, 8), 'c8'), ((1, 44, 46, 8), 'c8 at fwd8')],
}
# (dt, shape, positions): the launcher must refuse these and launch nothing
REFUSED_FWD = [('f32', (1, 43, 42, 8), True), ('f32', (1, 18, 93, 8), True), ('bf16', (1, 18, 93, 8), True), ('f32', (1, 45, 45, 8), False),
               ('bf16', (1, 45, 45, 24), False)]
REFUSED_BWD = [('f32', (1, 43, 42, 8)), ('f32', (1, 18, 93, 8)), ('bf16', (1, 18, 93, 16))]

FAMILIES = ('ties', 'const', 'zeros', 'nan1', 'nan_window', 'nan_corners', 'nan_plane', 'pinf', 'ninf_plane', 'ninf_border', 'ninf_but_one')
FAMILY_SHAPES = {'bf16': [(2, 12, 13, 32), (2, 12, 13, 16), (2, 12, 13, 8)], 'f32': [(2, 12, 13, 8)]}     # two trips of every plane walk


def family(name, dt, shape, seed=0):
    """the input of a case, as the float32 values of the tensor type"""
    N, H, W, C = shape
    rng = np.random.RandomState(100 + seed + 7 * H + W + C)
    x = rng.standard_normal(shape).astype(np.float32)
    big = H >= 8 and W >= 8
    assert big or name == 'random', 'the special families need a plane of 8 x 8 or more'
    if name == 'ties':
        x = np.round(x * 1.5) / 1.5
    elif name == 'const':
        x[:] = 0.5
    elif name == 'zeros':
        x = np.where(rng.rand(*shape) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
        x[:, :7, :7, 0] = -0.0                 # -0-only 5x5 windows around the outputs (0..4, 0..4) of level 1
        x[:, :, :, 1] = -0.0                   # and at every level
    elif name == 'nan1':
        x[0, H // 2, W // 2, 0] = np.nan
    elif name == 'nan_window':
        for h, w in ((5, 5), (5, 7), (6, 4), (7, 6), (7, 7)):
            x[0, h, w, 0] = np.nan
        x[N - 1, 3, 3:5, 2] = np.nan
    elif name == 'nan_corners':
        x[0, 0, 0, 1] = x[0, H - 1, W - 1, 1] = x[N - 1, 0, W - 1, 3] = x[N - 1, H - 1, 0, 3] = np.nan
    elif name == 'nan_plane':
        x[0, :, :, 0] = np.nan
    elif name == 'pinf':
        x[0, 0, 0, 0] = x[0, 6, 5, 0] = x[N - 1, H - 1, 3, 2] = np.inf
    elif name == 'ninf_plane':
        x[0, :, :, 0] = -np.inf
        x[N - 1, :, :, 5] = -np.inf
    elif name == 'ninf_border':
        x[:, :2, :, :] = -np.inf
        x[:, :, :2, :] = -np.inf
    elif name == 'ninf_but_one':
        x[:, :, :, :2] = -np.inf
        x[0, 3, 4, 0] = 1.25
        x[N - 1, 0, 0, 1] = -2.5
    else:
        assert name == 'random', name
    return q(x, dt)


def grads(dt, shape, integer=False, seed=0):
    """(g0, g1, g2, g3): the gradients of x's copy and of the three levels"""
    N, H, W, C = shape
    rng = np.random.RandomState(200 + seed + H + 3 * W)
    if integer:
        return [rng.randint(-8, 9, shape).astype(np.float32) for _ in range(4)]
    return [q(rng.standard_normal(shape), dt) for _ in range(4)]


def sppf_cases():
    """(id, dt, shape, family, layout, positions) of every SPPF case"""
    out = []
    for dt in DTYPES:
        for k, (shape, _) in enumerate(TRAIN[dt]):
            out.append((dt, shape, 'random', ('plan', 'wide')[k % 2], True))
        for k, (shape, _) in enumerate(INFER[dt]):
            out.append((dt, shape, 'random', ('wide', 'plan')[k % 2], False))
        for shape in FAMILY_SHAPES[dt]:
            for k, fam in enumerate(FAMILIES):
                out.append((dt, shape, fam, ('wide', 'plan')[k % 2], True))
    return [(f'{dt}-{"x".join(map(str, shape))}-{fam}-{lay}' + ('' if pos else '-infer'), dt, shape, fam, lay, pos) for dt, shape, fam, lay, pos in out]


# ------------------------------------------------------------------------------------------ upsample
UP_C = {'f32': (4, 24, 40), 'bf16': (8, 24, 40)}
UP_HW = ((1, 1), (5, 3), (6, 5))
UP_BIG_FWD = ('f32', (1, 64, 65, 256))        # 4 * 64 * 65 * 64 = 1064960 vectors
UP_BIG_BWD = ('f32', (1, 128, 129, 256))      # 128 * 129 * 64 = 1056768 vectors


def up_vectors(dt, shape, fwd):
    N, H, W, C = shape
    return N * H * W * (C // VE[dt]) * (4 if fwd else 1)


def upsample_cases():
    """(id, dt, (N, H, W, C) of the small side, pitched)"""
    out = []
    for dt in DTYPES:
        k = 0
        for C in UP_C[dt]:
            for H, W in UP_HW:
                out.append((f'{dt}-{1 + k % 3}x{H}x{W}x{C}' + ('-pitched' if k % 4 else ''), dt, (1 + k % 3, H, W, C), k % 4 != 0))
                k += 1
    return out


def up_input(dt, shape, seed, special=False, integer=False):
    rng = np.random.RandomState(300 + seed)
    if integer:
        return rng.randint(-8, 9, shape).astype(np.float32)
    a = q(rng.standard_normal(shape), dt)
    if special:
        flat = a.reshape(-1)
        flat[:: 17] = np.nan
        flat[3:: 19] = np.inf
        flat[5:: 23] = -np.inf
    return a


# ------------------------------------------------------------------------------------------ stem_prep, nchw_to_nhwc
STEM = [(1, 5, 7, 0), (2, 7, 5, 2), (3, 9, 11, 3), (1, 1, 1, 2), (2, 33, 17, 3)]        # (B, H, W, pad)
STEM_BIG = (1, 1020, 1021, 2)                                                         # 1024 * 1025 = 1049600 pixels
LAYOUT_C = (1, 3, 32, 33, 37, 64)
LAYOUT_HW = ((1, 1), (1, 31), (4, 8), (3, 11), (9, 11))                               # HW = 1, 31, 32, 33, 99


def image(shape, seed, special=True):
    rng = np.random.RandomState(400 + seed)
    a = (rng.standard_normal(shape) * 3).astype(np.float32)
    if special and a.size >= 8:
        flat = a.reshape(-1)
        flat[1] = np.nan
        flat[a.size // 2] = np.inf
        flat[-1] = -np.inf
        flat[a.size // 3] = -0.0
    return a
