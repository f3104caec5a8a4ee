"""Host side of the device augmentation (csrc/augment.hip): parameter draws, matrix composition, HSV tables and the packed cell table
that one upload per batch carries, plus the tile bank container.  No GPU is needed to import or run anything here except TileBank.to().

Reference: metayolo/datasets.py train_proc / TorchDataset.__getitem__ (training branch, keep_res <= 0), metayolo/engines/image_utils.py
random_transform_pars / estimate_matrix / random_hsv, datasets.py random_flip, image_utils.py get_crop_width(pos='random').  The
distributions are the reference's; the random stream is this project's (one numpy Generator per (seed, rank, epoch, step), mixed as
metayolo.datasets.SyntheticTiles mixes them) — the reference's global `random` / `np.random` streams are not reproduced.
"""
import math

import numpy as np

from . import _header

CELL_BYTES = _header.read().constants['HDY_AUG_CELL_BYTES']      # 24 words + three 256-byte tables
F_HFLIP, F_VFLIP, F_TRANSPOSE, F_HSV, F_PERSP = 1, 2, 4, 8, 16
MAX_K = 8
MAX_CELLS = 4096                       # B * k * k of one hdy_augment_boxes call
MAX_BOXES_PER_TILE = 65536
MASK_BACKGROUND = 0xFFFF               # an instance map's unowned pixels; a masked bank has at most 65535 boxes per tile
MASK_SIDE = 28                         # side of a mask target (target_to_tensors)
HYP_KEYS = ('degrees', 'translate', 'scale', 'shear', 'perspective', 'hsv_h', 'hsv_s', 'hsv_v', 'fliplr', 'flipud', 'transpose', 'cval',
            'k_mosaic', 'patch_size', 'img_size')


def step_seed(seed, rank, epoch, step):
    """the mixing of metayolo.datasets.SyntheticTiles"""
    return int(seed) + 1000003 * int(rank) + 7919 * int(epoch) + int(step)


def step_rng(seed, rank, epoch, step):
    return np.random.default_rng(step_seed(seed, rank, epoch, step))


def check_hyp(hyp):
    """The reference's keys; a missing one raises KeyError as `hyp[key]` does there.  Returns (k, patch, img_size, border byte)."""
    for key in HYP_KEYS:
        hyp[key]
    if hyp.get('color_aug', 'hsv') != 'hsv':
        raise ValueError(f"color_aug={hyp.get('color_aug')!r}: the device augmentation implements 'hsv' only")
    if hyp.get('keep_res', -1) > 0:
        raise ValueError('keep_res > 0 (resolution-preserving mosaic cells) is not implemented by the device augmentation')
    if hyp.get('albumentations') or hyp.get('albu'):
        raise ValueError('albumentations transforms are not implemented by the device augmentation')
    k, patch, size = int(hyp['k_mosaic']), int(hyp['patch_size']), int(hyp['img_size'])
    if not 1 <= k <= MAX_K:
        raise ValueError(f'k_mosaic={k}: 1 .. {MAX_K}')
    if patch < 4 or patch > 32768:
        raise ValueError(f'patch_size={patch}: 4 .. 32768')
    if size < 1 or size > k * patch:
        raise ValueError(f'img_size={size} exceeds the mosaic of k_mosaic * patch_size = {k * patch} pixels (the reference would return a smaller image)')
    return k, patch, size, border_byte(hyp['cval'])


def border_byte(cval):
    """cv2 hands a border value to an 8-bit image through saturate_cast<uchar>: round half to even, then clamp"""
    return int(min(max(np.rint(float(cval)), 0.0), 255.0))


def draw_params(rng, hyp, B, n_tiles):
    """One batch's parameters: arrays of shape (B, k*k) (cells in (r, c) order), `crop` (B, 2) = (x, y).  Distributions:
    random_transform_pars (uniform on the reference's intervals), random_hsv (applied with probability 0.5 when any gain is non-zero, gains
    uniform(-1, 1) * gain + 1), random_flip (one draw per flip), random.choices for the source tiles, get_crop_width(pos='random')."""
    k, patch, size, _ = check_hyp(hyp)
    if n_tiles < 1:
        raise ValueError('empty tile bank')
    shp = (B, k * k)
    u = lambda lo, hi: rng.uniform(lo, hi, shp)
    p = {'src': rng.integers(0, n_tiles, shp)}
    p['p_x'], p['p_y'] = u(-hyp['perspective'], hyp['perspective']), u(-hyp['perspective'], hyp['perspective'])
    p['angle'] = u(-hyp['degrees'], hyp['degrees'])
    p['scale'] = u(1 - hyp['scale'], 1 + hyp['scale'])
    p['shear_x'], p['shear_y'] = u(-hyp['shear'], hyp['shear']), u(-hyp['shear'], hyp['shear'])
    p['t_x'] = u(0.5 - hyp['translate'], 0.5 + hyp['translate']) * patch
    p['t_y'] = u(0.5 - hyp['translate'], 0.5 + hyp['translate']) * patch
    any_gain = bool(hyp['hsv_h'] or hyp['hsv_s'] or hyp['hsv_v'])
    p['hsv'] = (rng.random(shp) < 0.5) & any_gain
    p['hsv_gain'] = rng.uniform(-1, 1, shp + (3,)) * np.array([hyp['hsv_h'], hyp['hsv_s'], hyp['hsv_v']], np.float64) + 1
    p['hflip'] = rng.random(shp) < hyp['fliplr']
    p['vflip'] = rng.random(shp) < hyp['flipud']
    p['transpose'] = rng.random(shp) < hyp['transpose']
    p['crop'] = rng.integers(0, k * patch - size + 1, (B, 2))
    return p


def compose_matrices(p, tile_hw):
    """M = T @ (S @ R) @ P @ C of estimate_matrix for every cell, float64, shape (..., 3, 3).  R is cv2.getRotationMatrix2D(angle, (0, 0),
    scale) restated: [[a, b, 0], [-b, a, 0]] with a = scale cos(angle), b = scale sin(angle), angle in degrees."""
    shp = np.shape(p['angle'])
    eye = np.broadcast_to(np.eye(3), shp + (3, 3))
    C, P, R, S, T = (eye.copy() for _ in range(5))
    C[..., 0, 2], C[..., 1, 2] = -tile_hw[1] / 2, -tile_hw[0] / 2
    P[..., 2, 0], P[..., 2, 1] = p['p_x'], p['p_y']
    rad = np.asarray(p['angle'], np.float64) * (math.pi / 180)
    a, b = p['scale'] * np.cos(rad), p['scale'] * np.sin(rad)
    R[..., 0, 0], R[..., 0, 1], R[..., 1, 0], R[..., 1, 1] = a, b, -b, a
    S[..., 0, 1] = np.tan(np.asarray(p['shear_x'], np.float64) * math.pi / 180)
    S[..., 1, 0] = np.tan(np.asarray(p['shear_y'], np.float64) * math.pi / 180)
    T[..., 0, 2], T[..., 1, 2] = p['t_x'], p['t_y']
    return T @ (S @ R) @ P @ C


def hsv_luts(gain):
    """random_hsv's three tables exactly as numpy makes them there: (x r0) % 180, clip(x r1, 0, 255), clip(x r2, 0, 255), cast to uint8.
    gain (..., 3) float64 -> (..., 3, 256) uint8."""
    gain = np.asarray(gain, np.float64)
    x = np.arange(0, 256, dtype=np.float64)
    hue = ((x * gain[..., 0:1]) % 180).astype(np.uint8)
    sat = np.clip(x * gain[..., 1:2], 0, 255).astype(np.uint8)
    val = np.clip(x * gain[..., 2:3], 0, 255).astype(np.uint8)
    return np.stack([hue, sat, val], -2)


class CellTables:
    """`packed`: uint8 (n_cells * CELL_BYTES + B * 8,) — the cell records, then the crop offsets int32 (B, 2): one upload per batch.
    `cells` / `crop` are views of it; `M` / `Minv` the float64 matrices the fp32 words were rounded from."""

    def __init__(self, packed, B, k, M, Minv):
        self.packed, self.B, self.k, self.M, self.Minv = packed, B, k, M, Minv
        n = B * k * k
        self.cells = packed[:n * CELL_BYTES].reshape(n, CELL_BYTES)
        self.crop = packed[n * CELL_BYTES:].view(np.int32).reshape(B, 2)


def cell_tables(p, tile_hw, out=None):
    """Parameters -> the packed table (include/hdyolo.h, 'Cell table').  `out`: a uint8 array of the right size to fill (pinned memory)."""
    B, k2 = p['src'].shape
    k = int(round(math.sqrt(k2)))
    n = B * k2
    M = compose_matrices(p, tile_hw)
    Minv = np.linalg.inv(M)
    size = n * CELL_BYTES + B * 8
    packed = np.zeros(size, np.uint8) if out is None else out
    assert packed.dtype == np.uint8 and packed.shape == (size,)
    rec = packed[:n * CELL_BYTES].reshape(n, CELL_BYTES)
    words = rec[:, :96].view(np.int32)
    fwords = rec[:, :96].view(np.float32)
    words[:] = 0
    words[:, 0] = p['src'].reshape(n)
    fwords[:, 1:10] = Minv.reshape(n, 9).astype(np.float32)
    persp = M[..., 2, :2].reshape(n, 2).any(-1)
    flags = (p['hflip'].reshape(n) * F_HFLIP + p['vflip'].reshape(n) * F_VFLIP + p['transpose'].reshape(n) * F_TRANSPOSE +
             p['hsv'].reshape(n) * F_HSV + persp * F_PERSP)
    words[:, 10] = flags
    fwords[:, 11:20] = M.reshape(n, 9).astype(np.float32)
    fwords[:, 20] = p['scale'].reshape(n).astype(np.float32)
    rec[:, 96:] = hsv_luts(p['hsv_gain']).reshape(n, 768)
    packed[n * CELL_BYTES:].view(np.int32)[:] = np.asarray(p['crop'], np.int32).reshape(-1)
    return CellTables(packed, B, k, M, Minv)


def identity_params(B, k, tile, patch, src=0):
    """angle 0, scale 1, no shear, no perspective, t = 0.5 * patch, no flips, no HSV, crop (0, 0): with patch == tile the canvas is the tile"""
    shp = (B, k * k)
    z = np.zeros(shp)
    return {'src': np.full(shp, src, np.int64), 'p_x': z.copy(), 'p_y': z.copy(), 'angle': z.copy(), 'scale': z + 1, 'shear_x': z.copy(),
            'shear_y': z.copy(), 't_x': z + 0.5 * patch, 't_y': z + 0.5 * patch, 'hsv': np.zeros(shp, bool), 'hsv_gain': np.ones(shp + (3,)),
            'hflip': np.zeros(shp, bool), 'vflip': np.zeros(shp, bool), 'transpose': np.zeros(shp, bool), 'crop': np.zeros((B, 2), np.int64)}


class TileBank:
    """Source tiles and their boxes.  `.npz` format: tiles uint8 (n, H, W, 3); boxes float32 (M, 4) xyxy in pixels; labels int64 (M,) in
    1..nc; offsets int64 (n + 1,): tile t owns rows [offsets[t], offsets[t + 1]).  All tiles of a bank have one size.  Optional: instances
    uint16 (n, H, W), the instance map — a pixel holds the index of its object within its tile (bank row offsets[t] + value) or 0xFFFF for
    background; one owner per pixel (overlapping objects get partial masks), every pixel of an object inside its box grown to pixel edges.
    `has_mask` (uint8 per bank row: the object owns a pixel) is derived from it.  A `masks` array (any other mask format) is refused."""

    def __init__(self, tiles, boxes, labels, offsets, instances=None):
        tiles, boxes, labels, offsets = (np.asarray(a) for a in (tiles, boxes, labels, offsets))
        if tiles.dtype != np.uint8 or tiles.ndim != 4 or tiles.shape[3] not in (3, 4) or 0 in tiles.shape:
            raise ValueError(f'tile bank: tiles must be uint8 (n, H, W, 3) of one size, got {tiles.dtype} {tiles.shape} '
                             '(banks whose tiles differ in size are not supported)')
        n = tiles.shape[0]
        if boxes.ndim != 2 or boxes.shape[1] != 4 or boxes.dtype != np.float32:
            raise ValueError(f'tile bank: boxes must be float32 (M, 4) xyxy in pixels, got {boxes.dtype} {boxes.shape}')
        if labels.shape != (boxes.shape[0],) or labels.dtype != np.int64:
            raise ValueError(f'tile bank: labels must be int64 ({boxes.shape[0]},), got {labels.dtype} {labels.shape}')
        if offsets.shape != (n + 1,) or offsets.dtype != np.int64 or offsets[0] != 0 or offsets[-1] != boxes.shape[0] or (np.diff(offsets) < 0).any():
            raise ValueError(f'tile bank: offsets must be int64 ({n + 1},), non-decreasing from 0 to {boxes.shape[0]}')
        if not np.isfinite(boxes).all():
            raise ValueError('tile bank: non-finite box coordinate')
        if len(labels) and labels.min() < 1:
            raise ValueError('tile bank: labels are 1..nc (0 is the background class)')
        self.max_per_tile = int(np.diff(offsets).max()) if n else 0
        if self.max_per_tile > MAX_BOXES_PER_TILE:
            raise ValueError(f'tile bank: a tile with {self.max_per_tile} boxes (at most {MAX_BOXES_PER_TILE})')
        self.tiles, self.boxes, self.labels, self.offsets = tiles, boxes, labels, offsets
        self.n, self.H, self.W = n, tiles.shape[1], tiles.shape[2]
        self.nc = int(labels.max()) if len(labels) else 0
        self.device = None
        self.path = None                       # load() records where the bank came from, for messages
        self.instances, self.has_mask = None, None
        if instances is not None:
            self.instances, self.has_mask = self._check_instances(np.asarray(instances))

    def _check_instances(self, inst):
        """the instance map against the boxes; -> (map, has_mask uint8 (M,))"""
        if inst.dtype != np.uint16 or inst.shape != (self.n, self.H, self.W):
            raise ValueError(f'tile bank: instances must be uint16 {(self.n, self.H, self.W)} (one value per tile pixel), got {inst.dtype} {inst.shape}')
        if self.max_per_tile > MASK_BACKGROUND:
            raise ValueError(f'tile bank: a tile with {self.max_per_tile} boxes (at most {MASK_BACKGROUND} with an instance map: 0xFFFF is background)')
        has = np.zeros(len(self.boxes), np.uint8)
        for t in range(self.n):
            ys, xs = np.nonzero(inst[t] != MASK_BACKGROUND)
            if not len(ys):
                continue
            v = inst[t][ys, xs].astype(np.int64)
            lo, cnt = int(self.offsets[t]), int(self.offsets[t + 1] - self.offsets[t])
            if (v >= cnt).any():
                raise ValueError(f'tile bank: instances of tile {t} name object {int(v.max())}, the tile has {cnt} boxes')
            b = self.boxes[lo + v]
            inside = (np.floor(b[:, 0]) <= xs) & (xs < np.ceil(b[:, 2])) & (np.floor(b[:, 1]) <= ys) & (ys < np.ceil(b[:, 3]))
            if not inside.all():
                i = int(np.nonzero(~inside)[0][0])
                raise ValueError(f'tile bank: pixel ({int(xs[i])}, {int(ys[i])}) of tile {t} belongs to object {int(v[i])} but lies outside its box '
                                 f'{b[i].tolist()} grown to pixel edges')
            has[lo + np.unique(v)] = 1
        return inst, has

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            if 'masks' in z.files:
                raise ValueError("tile bank: a 'masks' array is not supported by the device augmentation (instance masks travel as the uint16 "
                                 "'instances' map)")
            missing = [key for key in ('tiles', 'boxes', 'labels', 'offsets') if key not in z.files]
            if missing:
                raise ValueError(f'tile bank {path}: missing arrays {missing}')
            bank = cls(z['tiles'], z['boxes'], z['labels'], z['offsets'], z['instances'] if 'instances' in z.files else None)
        bank.path = str(path)
        return bank

    def save(self, path):
        extra = {} if self.instances is None else {'instances': self.instances}
        np.savez(path, tiles=self.tiles, boxes=self.boxes, labels=self.labels, offsets=self.offsets, **extra)

    def to(self, device):
        """the bank as device tensors (uploaded once); returns self"""
        import torch
        dev = torch.device(device)
        self.d_tiles = torch.from_numpy(np.ascontiguousarray(self.tiles)).to(dev)
        nb = max(len(self.boxes), 1)                           # an annotation-free bank still hands the kernel valid pointers
        boxes, labels = np.zeros((nb, 4), np.float32), np.zeros((nb,), np.int64)
        boxes[:len(self.boxes)], labels[:len(self.labels)] = self.boxes, self.labels
        self.d_boxes, self.d_labels = torch.from_numpy(boxes).to(dev), torch.from_numpy(labels).to(dev)
        self.d_offsets = torch.from_numpy(np.ascontiguousarray(self.offsets)).to(dev)
        if self.instances is not None:
            self.d_instances = torch.from_numpy(np.ascontiguousarray(self.instances).view(np.int16)).to(dev)   # the map's bits (torch has no uint16 ops)
            has = np.zeros((nb,), np.uint8)
            has[:len(self.has_mask)] = self.has_mask
            self.d_has_mask = torch.from_numpy(has).to(dev)
        self.device = dev
        return self
