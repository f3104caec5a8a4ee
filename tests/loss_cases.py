"""The cases of the direct tests of the fused detection loss: geometries, target sets, logits and loss forms, and their restatement results
(tests/loss_ref.py), shared by test_loss_ref_host.py (which proves on the CPU that every case contains what it is for) and
test_gpu_loss_direct.py.  Everything is generated, as exact float32 values; nothing here imports hd_yolo_amd.

A case is named geometry-targets-logits-form, e.g. 'G3-latpile-sat-focal05'.
"""
import functools
import math

import numpy as np
import torch

import loss_ref

F32 = np.float32
ANCHOR_T = 4.0
HYP = {'box': 0.05, 'cls': 0.5, 'obj': 1.0, 'cls_pw': 1.0, 'obj_pw': 1.0, 'cls_cw': 1.0, 'fl_gamma': 0.0, 'anchor_t': ANCHOR_T,
       'label_smoothing': 0.0}
MODEL_ANCHORS_PX = [[10, 13, 16, 30, 33, 23], [30, 61, 62, 45, 59, 119], [116, 90, 156, 198, 373, 326]]
MODEL_STRIDES = [8, 16, 32]


def _model_anchors():
    return np.stack([np.asarray(a, F32).reshape(3, 2) / F32(s) for a, s in zip(MODEL_ANCHORS_PX, MODEL_STRIDES)])


def _g4_anchors():
    scale = [1.0, 0.8, 0.6, 0.4, 0.2]
    return np.asarray([[[0.6 * 1.25 ** k * s, 0.6 * 1.25 ** ((3 * k) % 8) * s] for k in range(8)] for s in scale], F32)


def _geom(name, grids, B, nc, ldl, ldg, anchors, strides=None):
    anchors = np.asarray(anchors, F32)
    nl, na = anchors.shape[:2]
    assert len(grids) == nl and ldl % 4 == 0 and ldg % 4 == 0 and min(ldl, ldg) >= na * (nc + 5)
    return {'name': name, 'nl': nl, 'na': na, 'grids': grids, 'B': B, 'nc': nc, 'no': nc + 5, 'ldl': ldl, 'ldg': ldg, 'anchors': anchors,
            'strides': strides or [2 ** l for l in range(nl)],
            'balance': {3: [4.0, 1.0, 0.4]}.get(nl, [4.0, 1.0, 0.25, 0.06, .02])[:nl]}


GEOMS = {g['name']: g for g in [
    _geom('G1', [(8, 8), (4, 4), (2, 2)], 2, 3, 24, 32, _model_anchors(), MODEL_STRIDES),            # the model's anchors
    _geom('G2', [(8, 8), (4, 4), (2, 2)], 2, 1, 20, 24, _model_anchors(), MODEL_STRIDES),            # 18 channels, no class term
    _geom('G3', [(6, 10), (3, 5)], 3, 2, 16, 16, [[[1, 1], [2, 4]], [[1, 2], [4, 4]]]),              # 14 channels, non-square, power-of-two anchors
    _geom('G4', [(16, 16), (8, 8), (4, 4), (2, 2), (1, 1)], 1, 4, 72, 80, _g4_anchors()),            # MAXL levels, MAXA anchors, a 1 x 1 level
    _geom('G5a', [(4, 4)], 1, 80, 256, 256, _model_anchors()[:1]),                                   # 255 channels
    _geom('G5b', [(4, 4)], 1, 128, 400, 400, _model_anchors()[:1]),                                  # MAXC classes, 399 channels
    _geom('G6', [(32, 32)], 4, 1, 8, 8, [[[2, 2]]]),                                                 # 212 000 targets
]}
G6_NT = 212000


# ------------------------------------------------------------------------------------------ targets
def class_rows(nt, nc):
    """one-hot, multi-hot, all-zero, one-hot, ... by row"""
    t = np.zeros((nt, nc), F32)
    for k in range(nt):
        if k % 4 != 2:
            t[k, (k if k % 4 < 2 else 7 * k) % nc] = 1
        if k % 4 == 1 and nc > 1:
            t[k, (k + 1) % nc] = 1
    return t


def _sizes(geom, k):
    """a box shape that some level's anchor accepts, cycling over levels, anchors and scale factors; normalised"""
    l = k % geom['nl']
    a = (k // geom['nl']) % geom['na']
    f = (0.8, 1.0, 1.5, 2.5, 0.4)[k % 5]
    ny, nx = geom['grids'][l]
    aw, ah = geom['anchors'][l][a]
    return min(float(aw) * f / nx, 1.0), min(float(ah) * f / ny, 1.0)


def lattice(geom):
    """every multiple of 1/16 in [0, 1]^2, borders included"""
    rows = []
    for iy in range(17):
        for ix in range(17):
            k = len(rows)
            rows.append((k % geom['B'], ix / 16.0, iy / 16.0) + _sizes(geom, k))
    return np.asarray(rows, F32)


PILE_N = 40
PILE_SAME = (0, 4, 30)               # identical rows: the largest IoU of the pile's cell, attained three times (the sort_obj_iou tie)


def pile_factors():
    hi = np.linspace(1.0, 0.8, PILE_N // 2)          # IoU with the planted prediction about f^2: 1 .. 0.64
    lo = np.linspace(0.35, 0.6, PILE_N // 2)         # 0.12 .. 0.36
    f = np.empty(PILE_N)
    f[0::2], f[1::2] = hi, lo
    f[list(PILE_SAME)] = 1.0
    return f


def pile(geom):
    """40 targets of image 0 with one centre in cell (gj 2, gi 3) of level 0, shapes f * (anchor 0 of level 0)"""
    ny, nx = geom['grids'][0]
    aw, ah = (float(v) for v in geom['anchors'][0][0])
    return np.asarray([(0, 3.25 / nx, 2.75 / ny, f * aw / nx, f * ah / ny) for f in pile_factors()], F32)


def _neighbours(c):
    c = F32(c)
    out = []
    if c > 0:
        out.append(('below', np.nextafter(c, F32(-1))))
    if c < 1:
        out.append(('above', np.nextafter(c, F32(2))))
    return out


def _edge_side(a, n, upper):
    """(side at the ratio threshold, side one step inside it): float32 w with fl(w * n) == 4 a (upper) or a / 4 exactly, and the nearest
    float32 towards the inside whose product differs"""
    a, fn = F32(a), F32(n)
    want = a * F32(ANCHOR_T) if upper else a / F32(ANCHOR_T)
    w = F32(want / fn)
    for _ in range(8):
        if w * fn == want:
            break
        w = np.nextafter(w, F32(2) if w * fn < want else F32(-1))
    else:
        raise AssertionError('no float32 side gives the threshold product exactly')
    inside = w
    while inside * fn == want:
        inside = np.nextafter(inside, F32(-1) if upper else F32(2))
    return float(w), float(inside)


def edges(geom):
    """centres one ulp off the cell and half-cell boundaries of level 0, sides at the anchor-ratio threshold of (level 0, anchor 0) and one
    step inside, degenerate rows; all in image 0 (with B > 1 the other images have no target).  Returns (rows, tags)."""
    ny, nx = geom['grids'][0]
    aw, ah = (float(v) for v in geom['anchors'][0][0])
    w0, h0 = 1.2 * aw / nx, 1.2 * ah / ny
    vx = [(s, h, v) for k in range(nx + 1) for h in (0, 1) if (k + h / 2) / nx <= 1 for s, v in _neighbours((k + h / 2) / nx)]
    vy = [(s, h, v) for k in range(ny + 1) for h in (0, 1) if (k + h / 2) / ny <= 1 for s, v in _neighbours((k + h / 2) / ny)]
    rows, tags = [], {'ulp_x': [], 'ulp_y': [], 'ratio': [], 'degenerate': []}
    for i, (s, h, v) in enumerate(vx):
        tags['ulp_x'].append((len(rows), s, h))
        rows.append((0, v, vy[(5 * i + 3) % len(vy)][2], w0, h0))
    for i, (s, h, v) in enumerate(vy):
        tags['ulp_y'].append((len(rows), s, h))
        rows.append((0, vx[(3 * i + 1) % len(vx)][2], v, w0, h0))
    for dim, (a, n) in enumerate(((aw, nx), (ah, ny))):
        for upper in (True, False):
            at, inside = _edge_side(a, n, upper)
            if at > 1:
                continue
            for side in (at, inside):
                rows.append((0, 0.5 + 0.25 / nx, 0.5 + 0.25 / ny) + ((side, ah / ny) if dim == 0 else (aw / nx, side)))
            tags['ratio'].append((len(rows) - 2, len(rows) - 1))
    for w, h in ((0.0, h0), (w0, 0.0), (0.0, 0.0)):
        tags['degenerate'].append(len(rows))
        rows.append((0, 0.4, 0.6, w, h))
    return np.asarray(rows, F32), tags


def g6_targets(geom):
    """centres on a 1/64 lattice (the cell and half-cell boundaries of the 32-grid), three quarters of them jittered off it; sides within
    the anchor's ratio band"""
    rng = np.random.default_rng(6)
    nt = G6_NT
    c = rng.integers(0, 65, (nt, 2)).astype(np.float64) / 64
    jit = rng.uniform(-0.3, 0.3, (nt, 2)) / 64 * (rng.random((nt, 1)) < 0.75)
    c = np.clip(c + jit, 0, 1)
    wh = 2.0 / 32 * rng.uniform(0.3, 3.5, (nt, 2))
    return np.concatenate([rng.integers(0, geom['B'], (nt, 1)).astype(np.float64), c, wh], 1).astype(F32)


@functools.lru_cache(maxsize=None)
def targets_of(gname, tset):
    """(gts (nt, 5) float32, tcls (nt, nc) float32, tags)"""
    geom = GEOMS[gname]
    tags = {}
    if tset == 'latpile':
        lat = lattice(geom)
        gts = np.concatenate([lat, pile(geom)])
        tags['pile'] = len(lat)
    elif tset == 'small':
        gts = lattice(geom)[20:27]
    elif tset == 'edges':
        gts, tags = edges(geom)
    elif tset == 'g6':
        gts = g6_targets(geom)
    else:
        assert tset == 'empty'
        gts = np.zeros((0, 5), F32)
    return np.ascontiguousarray(gts, F32), class_rows(len(gts), geom['nc']), tags


# ------------------------------------------------------------------------------------------ logits
def _logit(s):
    return math.log(s / (1 - s))


def plant(x, geom, l, b, a, gj, gi, tbox, mode):
    """Solve the four box logits of (level l, image b, cell, anchor a) so that the predicted box is the target shrunk by 2e-4 ('equal':
    IoU > 0.999, v = 0; strictly inside, so no min / max of the CIoU sits on a knife edge of float32 rounding; for the same
    reason the other constants are not round numbers: the lattice targets sharing the cell have edges on round numbers), the target at 0.5317 of its size
    ('aspect': v = 0; not one half, whose edges fall on the lattice targets' edges) or a small box clear of it ('outside': intersection 0).  False when the cell cannot express it."""
    tx, ty, gw, gh = (float(v) for v in tbox)
    aw, ah = (float(v) for v in geom['anchors'][l][a])
    if mode == 'equal':
        px, py, w, h = tx, ty, gw * (1 - 2e-4), gh * (1 - 2e-4)
    elif mode == 'aspect':
        px, py, w, h = tx, ty, gw * 0.5317, gh * 0.5317
    else:
        w, h, px = 0.0413 * aw, 0.0413 * ah, None
        for qx, qy in ((-0.4437, -0.4437), (1.4437, 1.4437), (-0.4437, 1.4437), (1.4437, -0.4437)):
            if abs(qx - tx) > (w + gw) / 2 + 0.05 or abs(qy - ty) > (h + gh) / 2 + 0.05:
                px, py = qx, qy
                break
        if px is None:
            return False
    s = [(px + 0.5) / 2, (py + 0.5) / 2, math.sqrt(w / aw) / 2, math.sqrt(h / ah) / 2]
    if not all(0.01 < v < 0.99 for v in s):
        return False
    no = geom['no']
    x[b, gj, gi, a * no:a * no + 4] = torch.tensor([_logit(v) for v in s], dtype=torch.float32)
    return True


SAT_VALUES = np.asarray([17, -17, 88, -88, 100, -100], F32)


@functools.lru_cache(maxsize=None)
def logits_of(gname, tset, kind):
    """per level (B, ny, nx, ldl) float32, padding channels random too.  'u1' / 'u12': uniform; 'sat': +-12 with 15 % of the entries from
    SAT_VALUES; 'planted': +-1 with every third candidate's box logits solved (plant), modes in turn.  Whenever the targets hold the pile,
    its centre cell on level 0, anchor 0, predicts the pile's first box."""
    geom = GEOMS[gname]
    gts, _, tags = targets_of(gname, tset)
    rng = np.random.default_rng([ord(ch) for ch in gname + tset + kind])
    amp = {'u1': 1.0, 'u12': 12.0, 'sat': 12.0, 'planted': 1.0}[kind]
    out = []
    for l, (ny, nx) in enumerate(geom['grids']):
        shape = (geom['B'], ny, nx, geom['ldl'])
        x = rng.uniform(-amp, amp, shape).astype(F32)
        if kind == 'sat':
            x = np.where(rng.random(shape) < 0.15, SAT_VALUES[rng.integers(0, len(SAT_VALUES), shape)], x).astype(F32)
        x = torch.from_numpy(x)
        if len(gts) and (kind == 'planted' or (l == 0 and 'pile' in tags)):
            m = loss_ref.match_level(gts, geom['anchors'][l], ny, nx, ANCHOR_T)
            if kind == 'planted':
                for c in range(0, len(m['g']), 3):
                    plant(x, geom, l, m['b'][c], m['a'][c], m['gj'][c], m['gi'][c], m['tbox'][c], ('equal', 'outside', 'aspect')[(c // 3) % 3])
            if l == 0 and 'pile' in tags:
                c = np.nonzero((m['g'] == tags['pile']) & (m['j'] == 0) & (m['a'] == 0))[0]
                assert len(c) == 1 and plant(x, geom, 0, m['b'][c[0]], 0, m['gj'][c[0]], m['gi'][c[0]], m['tbox'][c[0]], 'equal')
        out.append(x.contiguous())
    return out


# ------------------------------------------------------------------------------------------ loss forms
def _per_class(nc, vals):
    return [vals[c % len(vals)] for c in range(nc)]


def form_of(form, nc):
    """(hyp for DetLoss, gr, sort_obj_iou)"""
    hyp = dict(HYP)
    gr, sort = 1.0, False
    if form == 'smooth':
        hyp.update(label_smoothing=0.1, cls_pw=_per_class(nc, [1.0, 2.0, 0.5]), cls_cw=_per_class(nc, [1.0, 0.5, 2.0]), obj_pw=0.7)
    elif form == 'focal15':
        hyp['fl_gamma'] = 1.5
    elif form == 'focal05':
        hyp['fl_gamma'] = 0.5
    elif form == 'gr05':
        gr = 0.5
    elif form == 'gr0':
        gr = 0.0
    elif form == 'sort':
        sort = True
    elif form == 'sort_gr05':
        gr, sort = 0.5, True
    else:
        assert form == 'bce'
    return hyp, gr, sort


def class_weights(hyp, nc):
    """cls_cw and cls_pw as lists of nc"""
    def wide(v):
        return [float(x) for x in v] if isinstance(v, (list, tuple)) else [float(v)] * nc
    return wide(hyp['cls_cw']), wide(hyp['cls_pw'])


def _cases():
    names = []
    for g in ('G1', 'G2', 'G3', 'G4', 'G5a', 'G5b'):
        for tset in ('latpile', 'edges'):
            names += [f'{g}-{tset}-{kind}-bce' for kind in ('u1', 'u12', 'sat', 'planted')]
        names.append(f'{g}-empty-u1-bce')
    names += ['G1-small-u12-bce', 'G6-g6-u1-bce']
    for g in ('G1', 'G3'):
        names += [f'{g}-latpile-u12-smooth', f'{g}-latpile-u12-focal15', f'{g}-latpile-sat-focal05', f'{g}-latpile-u12-gr05',
                  f'{g}-latpile-u12-gr0', f'{g}-latpile-u12-sort', f'{g}-latpile-u12-sort_gr05']
    return names


CASES = _cases()
HARD = [n for n in CASES if n.split('-')[2] in ('sat', 'planted')]       # saturated or planted logits: the yardstick rule may apply


@functools.lru_cache(maxsize=None)
def inputs_of(name):
    gname, tset, kind, form = name.split('-')
    geom = GEOMS[gname]
    gts, tcls, tags = targets_of(gname, tset)
    hyp, gr, sort = form_of(form, geom['nc'])
    return {'geom': geom, 'gts': gts, 'tcls': tcls, 'tags': tags, 'logits': logits_of(gname, tset, kind), 'hyp': hyp, 'gr': gr, 'sort': sort}


@functools.lru_cache(maxsize=None)
def ref_of(name, dtype=torch.float64):
    """loss_ref.det_loss of a case (computed once per process and dtype; callers must not modify it)"""
    c = inputs_of(name)
    geom, hyp = c['geom'], c['hyp']
    cw, pw = class_weights(hyp, geom['nc'])
    return loss_ref.det_loss(c['logits'], c['gts'], c['tcls'], geom['anchors'], geom['nc'], geom['balance'], cw, pw, hyp['obj_pw'],
                             hyp['anchor_t'], hyp['label_smoothing'], hyp['box'], hyp['obj'], hyp['cls'], hyp['fl_gamma'], 0.25, c['gr'],
                             c['sort'], dtype=dtype)


def elementwise(got, ref, rtol=1e-4):
    """the project's gradient criterion (tests/test_gpu_loss_forms.py): the worst |error| - rtol * |ref| in units of rms(ref)"""
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    rms = ref.pow(2).mean().sqrt().item() + 1e-30
    return ((got - ref).abs() - rtol * ref.abs()).max().item() / rms
