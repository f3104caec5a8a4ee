"""Named inputs for the direct tests of csrc/detect.hip (tests/test_gpu_detect_direct.py); tests/test_detect_ref_host.py proves on the CPU
what each contains.  Plain numpy, seeded, made on the CPU.

Decode.  DECODE_LAYOUTS names (B, na, ny, nx, no, pitch); each is run in three forms of the same values: 'pixel' ([B][ny][nx][pitch] with
channel a no + o, the plan's layout), 'contig' ((B, na, ny, nx, no) contiguous) and 'permuted' (storage (na, B, nx, ny, no): a view whose four
outer strides are all out of order; o stays contiguous, which the ABI requires).  `takes_tiled` restates hdy_decode's predicate; `decode_path`
names the kernel path a form must take: 'tiled first branch' (no + 1 <= 16), 'tiled second branch', or 'per-candidate'.  DECODE_FALLBACKS are
pixel-major inputs the predicate must refuse (pitch 68, pitch 27, a base that is 4- but not 16-byte aligned).  DECODE_LARGE are the two inputs
above the grid caps of 2048 workgroups x 128 pixels and 4096 x 256 candidates.  Fills: 'randn' (4 N(0, 1)) and 'sweep' (SWEEP written cyclically
over all positions in (b, a, y, x, o) order; its length 31 is prime, so with at least 31 pixels every anchor and column meets every value).
Padding channels hold NaN.

NMS.  Every generator returns a dict with preds (B, N, 5 + nc + extra) and the arguments of hdy_nms_batched.  Rows are
(cx, cy, w, h, obj, cls..., extra); the extra column carries the row number, so a gathered row names its source.

det_outputs and det_grad_pack: see the generators.
"""
import numpy as np

NAN, INF = float('nan'), float('inf')

# ------------------------------------------------------------------------------------------ decode
DECODE_LAYOUTS = {
    'a': (2, 3, 12, 20, 7, 24),
    'b': (1, 3, 9, 7, 5, 16),         # no = 5, the ABI minimum
    'c': (3, 3, 5, 3, 9, 28),         # pitch a multiple of 4, not of 8
    'd': (2, 3, 11, 13, 15, 48),      # row = 16: the last of the first tiled branch
    'e': (2, 3, 11, 13, 16, 48),      # no padding; row = 17: the second branch
    'f': (2, 3, 6, 10, 21, 64),       # the upper pitch limit
    'g': (2, 1, 8, 8, 13, 16),
    'h': (1, 8, 4, 6, 8, 64),
    'i': (2, 8, 3, 5, 5, 40),
    'j': (20, 3, 3, 5, 7, 24),        # one 128-pixel tile spans 8 images
    'k': (1, 3, 1, 1, 7, 24),         # one pixel
    'l': (1, 3, 3, 5, 7, 24),         # fewer than 16 pixels
}
FORMS = ('pixel', 'contig', 'permuted')
FILLS = ('randn', 'sweep')
DECODE_FALLBACKS = {
    'pitch68': (2, 3, 5, 7, 22, 68),          # pitch above 64
    'pitch27': (3, 3, 5, 3, 9, 27),           # pitch not a multiple of 4 (exactly na no)
    'misaligned': (2, 3, 12, 20, 7, 24),      # case a, base moved by one float
}
DECODE_LARGE = {
    'tiled': (1, 3, 515, 510, 7, 24),         # 262650 pixels > 2048 x 128
    'percand': (1, 3, 600, 583, 7, 7),        # 1049400 candidates > 4096 x 256, contiguous
}
DEC_TP, DEC_TILE_GRID, DEC_CAND_GRID = 128, 2048, 4096 * 256

_PAIRS = [v for p in (0, 1, 20, 80, 87, 87.5, 88, 88.7, 89, 100) for v in (p, -p)]
SWEEP = np.array([0.0, -0.0, 1e-30, -1e-30, 1e-3, -1e-3] + _PAIRS[2:] + [1e4, -1e4, 3e38, -3e38, INF, -INF, NAN], np.float32)
assert len(SWEEP) == 31

ANCHORS_P5 = [[10, 13, 16, 30, 33, 23], [30, 61, 62, 45, 59, 119], [116, 90, 156, 198, 373, 326]]
ANCHORS_FRAC = [1.25, 3.5, 2.75, 1.5, 6.125, 9.75, 12.5, 7.25, 20.75, 33.5, 41.25, 18.5, 70.5, 55.25, 90.125, 130.75]
STRIDES = (8.0, 16.0, 32.0, 64.0)


def anchors_and_stride(k, na):
    """case number -> (2 na anchor sides in pixels, stride): the P5 levels and the fractional set in turn, the four strides in turn"""
    pool = [ANCHORS_P5[0] + ANCHORS_P5[1] + ANCHORS_P5[2][:4], ANCHORS_FRAC, ANCHORS_P5[1] + ANCHORS_P5[2] + ANCHORS_P5[0][:4],
            ANCHORS_FRAC[::-1]][k % 4]
    return [float(v) for v in pool[:2 * na]], STRIDES[k % 4]


def decode_setup(name):
    """layout name -> (shape tuple, anchors, stride, level id)"""
    names = list(DECODE_LAYOUTS) + list(DECODE_FALLBACKS) + list(DECODE_LARGE)
    k = names.index('a' if name == 'misaligned' else name)        # 'misaligned' is case a itself: the same values, anchors and stride
    spec = {**DECODE_LAYOUTS, **DECODE_FALLBACKS, **DECODE_LARGE}[name]
    anc, st = anchors_and_stride(k, spec[1])
    return spec, anc, st, k % 5


def decode_values(name, fill):
    """the logical logits (B, na, ny, nx, no) fp32"""
    (B, na, ny, nx, no, _), _, _, k = decode_setup(name)
    n = B * na * ny * nx * no
    if fill == 'sweep':
        return SWEEP[np.arange(n) % len(SWEEP)].reshape(B, na, ny, nx, no).copy()
    rng = np.random.default_rng(1000 + 7 * k)
    return (rng.standard_normal(n, dtype=np.float32) * np.float32(4)).reshape(B, na, ny, nx, no)


def strides_of(form, B, na, ny, nx, no, pitch):
    """element strides (sb, sa, sy, sx) of the view handed to hdy_decode, and the floats the storage holds"""
    if form == 'pixel':
        return (ny * nx * pitch, no, nx * pitch, pitch), B * ny * nx * pitch
    if form == 'contig':
        return (na * ny * nx * no, ny * nx * no, nx * no, no), B * na * ny * nx * no
    if form == 'permuted':                                     # storage (na, B, nx, ny, no)
        return (nx * ny * no, B * nx * ny * no, no, ny * no), B * na * ny * nx * no
    raise KeyError(form)


def takes_tiled(strides, na, ny, nx, no, aligned16=True):
    """hdy_decode's predicate for the tiled kernel, restated"""
    sb, sa, sy, sx = strides
    return bool(sa == no and sy == nx * sx and sb == ny * sy and sx % 4 == 0 and sx >= na * no and sx <= 64 and aligned16)


def decode_path(name, form):
    spec = {**DECODE_LAYOUTS, **DECODE_FALLBACKS, **DECODE_LARGE}[name]
    B, na, ny, nx, no, pitch = spec
    st, _ = strides_of(form, *spec)
    if takes_tiled(st, na, ny, nx, no, aligned16=name != 'misaligned'):
        return 'tiled first branch' if no + 1 <= 16 else 'tiled second branch'
    return 'per-candidate'


# ------------------------------------------------------------------------------------------ NMS
SURVIVORS = (0, 1, 63, 64, 65, 1023, 1024, 1025, 8191, 8192, 8193)
NMS_LDS_KEEP = 4096


def _rows(rng, n, nc, side, lo=12.0, hi=30.0):
    """n random rows: centres in a square of `side`, sides lo..hi, obj and class scores in (0, 1), one extra column with the row number"""
    p = np.empty((n, 5 + nc + 1), np.float32)
    p[:, 0:2] = rng.uniform(0, side, (n, 2))
    p[:, 2:4] = rng.uniform(lo, hi, (n, 2))
    p[:, 4:5 + nc] = rng.uniform(0.0, 1.0, (n, 1 + nc))
    p[:, 5 + nc] = np.arange(n)
    return p


def case(preds, nc, conf, iou, max_det, min_wh=2.0, class_aware=False):
    preds = np.ascontiguousarray(preds, np.float32)
    if preds.ndim == 2:
        preds = preds[None]
    return {'preds': preds, 'nc': nc, 'conf': conf, 'iou': iou, 'max_det': max_det, 'min_wh': min_wh, 'class_aware': class_aware}


FILTER_MIN_WH = (2.0, 0.0, 3.5)


def nms_filter_edges(min_wh):
    """integer centres, w and h = min_wh + {-0.5, 0, 0, +0.5} independently: every difference x2 - x1 is exact, so a side either equals
    min_wh (kept by >=), lies half a pixel below (rejected) or above"""
    rng = np.random.default_rng(int(min_wh * 10) + 21)
    B, N, nc = 2, 3000, 2
    p = np.stack([_rows(rng, N, nc, 1024.0) for _ in range(B)])
    p[..., 0:2] = rng.integers(0, 1024, (B, N, 2))
    p[..., 2:4] = np.float32(min_wh) + np.array([-0.5, 0.0, 0.0, 0.5], np.float32)[rng.integers(0, 4, (B, N, 2))]
    p[..., 4] = rng.uniform(0.3, 1.0, (B, N))                 # everything above conf: the size filter alone decides
    return case(p, nc, 0.25, 0.45, N, min_wh=min_wh)


STRICT_CONF = (0.0, 0.25, 1.0)


def nms_strict_conf(conf):
    """a third of the scores exactly conf, a third the next float above, a third the next float below"""
    rng = np.random.default_rng(31)
    N, nc = 3000, 1
    p = _rows(rng, N, nc, 3000.0)
    c = np.float32(conf)
    p[:, 4] = np.array([c, np.nextafter(c, np.float32(INF)), np.nextafter(c, np.float32(-INF))], np.float32)[np.arange(N) % 3]
    return case(p, nc, conf, 0.45, 1500)


IOU_SETS = ('dense', 'duplicates')


def nms_iou(kind, iou):
    rng = np.random.default_rng(41)
    N, nc = 2000, 1
    if kind == 'dense':
        p = _rows(rng, N, nc, 300.0)
    else:
        p = _rows(rng, N // 2, nc, 4000.0)
        p = np.concatenate([p, p])[rng.permutation(N)]         # every box twice, exactly
        p[:, 5 + nc] = np.arange(N)
    p[:, 4] = rng.uniform(0.3, 1.0, N)
    return case(p, nc, 0.25, iou, N)


def survivor_rows(M, seed, n_low=500, N=None):
    """M rows above conf = 0.25, sparse (side 45 sqrt(M) + 100, sides 12..30), and n_low (or N - M) rows below it, interleaved"""
    rng = np.random.default_rng(seed)
    N = M + n_low if N is None else N
    p = _rows(rng, N, 1, 45.0 * np.sqrt(max(M, 1)) + 100.0)
    above = np.zeros(N, bool)
    above[rng.permutation(N)[:M]] = True
    p[:, 4] = np.where(above, rng.uniform(0.3, 1.0, N), rng.uniform(0.0, 0.2, N))
    return p


def survivor_max_dets(M):
    md = [max(M, 1), 300]
    if M >= NMS_LDS_KEEP:
        md += [NMS_LDS_KEEP, NMS_LDS_KEEP + 1]
    return md


def nms_survivors(M, max_det):
    return case(survivor_rows(M, 50 + M), 1, 0.25, 0.45, max_det)


def kept_list(max_det):
    return 'LDS kept list' if max_det <= NMS_LDS_KEEP else 'workspace kept list'


MIXED_B = 64


def mixed_counts():
    """per-image survivor counts of the mixed batch: every count of SURVIVORS once, two images with nothing above conf (-1 marks them; like
    0, but listed on their own), the rest drawn from the counts up to 1025"""
    rng = np.random.default_rng(61)
    counts = list(SURVIVORS) + [-1, -1]
    counts += [int(v) for v in rng.choice(SURVIVORS[:8], MIXED_B - len(counts))]
    return [counts[i] for i in rng.permutation(MIXED_B)]


def nms_mixed_batch(max_det=300):
    N = max(SURVIVORS) + 500
    p = np.stack([survivor_rows(max(m, 0), 70 + i, N=N) for i, m in enumerate(mixed_counts())])
    return case(p, 1, 0.25, 0.45, max_det)


def nms_empty_rows():
    return case(np.zeros((3, 0, 7), np.float32), 1, 0.25, 0.45, 300)


PRECUT = 30000
PRECUT_ISOLATED = 40


def nms_precut(below=False):
    """class-aware, N = 33000: 1200 rows of objectness 0.1, 40 isolated boxes (obj 0.26, class scores 1.0) far from a dense cluster of 31760
    rows (centres in a 60 x 60 square, sides 30..40; 600 of them pass on objectness and fail on obj x class).  States: (i) more than 30000 rows pass both thresholds, (ii) every isolated box ranks
    beyond 30000, (iii) the oracle keeps fewer than max_det, (iv) with `below` (1500 cluster rows lowered to objectness 0.1) fewer than
    30000 pass and all isolated boxes are kept.  Returns (case, rows of the isolated boxes)."""
    rng = np.random.default_rng(81)
    N, nc = 33000, 3
    p = _rows(rng, N, nc, 60.0, 30.0, 40.0)
    p[:, 4] = rng.uniform(0.4, 1.0, N)                        # cluster: obj * best class >= 0.28, above the isolated boxes' 0.26
    p[:, 5:5 + nc] = rng.uniform(0.7, 1.0, (N, nc))
    perm = rng.permutation(N)
    low, iso, extra_low, weak = perm[:1200], np.sort(perm[1200:1200 + PRECUT_ISOLATED]), perm[1240:1240 + 1500], perm[2740:2740 + 600]
    p[low, 4] = 0.1
    p[weak, 4] = 0.3                                           # 600 rows pass obj > conf and fail obj * cls > conf (0.24)
    p[weak, 5:5 + nc] = 0.8
    p[iso, 0] = 2000.0 + 100.0 * np.arange(PRECUT_ISOLATED)
    p[iso, 1] = 3000.0
    p[iso, 2:4] = 30.0
    p[iso, 4] = 0.26
    p[iso, 5:5 + nc] = 1.0
    if below:
        p[extra_low, 4] = 0.1
    return case(p, nc, 0.25, 0.45, 1000, class_aware=True), iso


def nms_class_offsets():
    """nc = 80, best classes spread over 0..79 (offset up to 79 x 7680 = 606720: the shifted coordinates round to 1/16 px), pairs of identical
    boxes with the same best class (rows 4i, 4i + 1) and with different best classes (4i + 2, 4i + 3), best-class ties every 5th row"""
    rng = np.random.default_rng(91)
    B, N, nc = 2, 1500, 80
    p = np.stack([_rows(rng, N, nc, 640.0) for _ in range(B)])
    p[..., 4] = rng.uniform(0.5, 1.0, (B, N))
    p[..., 5:5 + nc] = rng.uniform(0.0, 0.5, (B, N, nc))
    best = (np.arange(N) * 37 + np.arange(N) // 4) % nc
    for b in range(B):
        p[b, np.arange(N), 5 + best] = 0.9
        p[b, 1::4, :4] = p[b, 0::4, :4]                       # the same box ...
        p[b, 1::4, 5:5 + nc] = p[b, 0::4, 5:5 + nc]           # ... and the same best class: one of the two goes
        p[b, 3::4, :4] = p[b, 2::4, :4][:len(p[b, 3::4])]     # the same box, another best class: both stay unless something else takes them
        tie = np.arange(0, N, 5)
        p[b, tie, 5 + (best[tie] + 11) % nc] = 0.9            # a second class at the maximum: the first (lower) one wins
    return case(p, nc, 0.25, 0.45, 1000, class_aware=True)


def nms_nonfinite():
    """every 7th row has one of its first five columns set to NaN, +inf or -inf in rotation (all 15 combinations occur)"""
    rng = np.random.default_rng(101)
    B, N, nc = 2, 2000, 2
    p = np.stack([_rows(rng, N, nc, 900.0) for _ in range(B)])
    vals = np.array([NAN, INF, -INF], np.float32)
    for b in range(B):
        for k, r in enumerate(range(b, N, 7)):
            p[b, r, k % 5] = vals[k % 3]
    return case(p, nc, 0.25, 0.45, 2000)


def xyxy_survivors(M):
    """boxes (M, 4) xyxy and scores (M,) for ops.nms: the geometry of survivor_rows"""
    p = survivor_rows(M, 150 + M, n_low=0)
    hw, hh = p[:, 2] / np.float32(2), p[:, 3] / np.float32(2)
    return np.stack([p[:, 0] - hw, p[:, 1] - hh, p[:, 0] + hw, p[:, 1] + hh], 1).astype(np.float32), p[:, 4].copy()


# ------------------------------------------------------------------------------------------ det_outputs
TREE = {1: [2, 3], 5: [6], 0: [1, 2, 3, 4, 5, 6]}               # 0 -> {1 -> {2, 3}, 4, 5 -> {6}}: children before their parent
TREE_PAIRS = [(c, k) for k, v in TREE.items() for c in v]
OUT_CONF = 0.2
OUT_CASES = [(B, nc, tree, edge_empty) for B in (1, 7, 300) for nc, tree in ((1, False), (6, False), (6, True)) for edge_empty in (False, True)
             if not (B == 1 and edge_empty)]


def det_outputs_case(B, nc, tree, edge_empty):
    """scores (B, max_det, 1 + nc), boxes, n_keep mixing 0, 1, max_det and random counts (first and last image empty with `edge_empty`).
    Special rows, by j % 16 within an image: 3 a tie between two classes; 5 every class score equal to conf and objectness 1 (no hit; with the
    tree the products fall below conf); 7 NaN in the first class column; 9 NaN in a later class column with a finite score above conf elsewhere;
    11 NaN objectness; 13 (nc > 1) objectness and the inner nodes 1, the leaves equal to conf."""
    rng = np.random.default_rng(200 + 13 * B + nc + 2 * tree + edge_empty)
    max_det = 12 if B == 300 else 40
    C = 1 + nc
    n_keep = rng.integers(0, max_det + 1, B).astype(np.int32)
    n_keep[::4], n_keep[1::4] = max_det, 1
    n_keep[2::8] = 0
    if edge_empty:
        n_keep[0] = n_keep[-1] = 0
    elif B > 1:
        n_keep[0], n_keep[-1] = max_det, max_det - 1
    scores = rng.uniform(0.0, 1.0, (B, max_det, C)).astype(np.float32)
    boxes = rng.uniform(0.0, 100.0, (B, max_det, 4)).astype(np.float32)
    j = np.arange(max_det)
    cf = np.float32(OUT_CONF)
    if nc > 1:
        scores[:, j % 16 == 3, 3] = scores[:, j % 16 == 3, 2]
        scores[:, j % 16 == 9, nc] = NAN
        scores[:, j % 16 == 9, 1] = 0.95
        scores[:, j % 16 == 9, 0] = 1.0
        scores[:, j % 16 == 13, :] = cf
        scores[:, j % 16 == 13, 0] = 1.0
        scores[:, j % 16 == 13, 1] = 1.0
        scores[:, j % 16 == 13, 5 if nc >= 5 else 1] = 1.0
    scores[:, j % 16 == 5, 1:] = cf
    scores[:, j % 16 == 5, 0] = 1.0
    scores[:, j % 16 == 7, 1] = NAN
    scores[:, j % 16 == 11, 0] = NAN
    return {'scores': scores, 'boxes': boxes, 'n_keep': n_keep, 'max_det': max_det, 'nc': nc, 'pairs': TREE_PAIRS if tree else [],
            'conf': OUT_CONF}


# ------------------------------------------------------------------------------------------ det_grad_pack
PACK_GRID = 8192 * 256
PACK_SHAPES = [((2, 3, 7, 9, 13), 39), ((2, 3, 7, 9, 13), 40), ((2, 3, 7, 9, 13), 48), ((1, 1, 1, 1, 5), 8), ((1, 8, 2, 3, 8), 64),
               ((1, 3, 9, 5419, 13), 43)]               # the last: 9 x 5419 x 43 = 8192 x 256 + 1 elements, one more than the largest grid
PACK_FORMS = ('pixel', 'contig', 'ostride')
PACK_SPECIALS = np.array([0.0, -0.0, NAN, INF, -INF,
                          1.00390625, 1.01171875, -1.00390625, -1.01171875,      # halfway between two bf16 values: 1 + 2^-8 (down to even), 1 + 3 x 2^-8 (up)
                          1.00390637, 1.00390613, 3.3895314e38, 3.4028235e38, 1e-40, -1e-40], np.float32)


def grad_pack_values(shape, seed=0):
    rng = np.random.default_rng(300 + seed)
    n = int(np.prod(shape))
    g = rng.standard_normal(n, dtype=np.float32)
    at = np.arange(0, n, 11)
    g[at] = PACK_SPECIALS[np.arange(len(at)) % len(PACK_SPECIALS)]
    return g.reshape(shape)
