"""Instance masks through the device augmentation, the parts that need no GPU: the bank format (hd_yolo_amd.augment.TileBank with an instance
map, synth.synth_tile_bank(instances=True)), the argument checks of the three entry points of csrc/augment_masks.hip (they return before any
launch), and the CPU restatement tests/augment_mask_ref.py on its own: identity, flips, no masked object."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import augment_mask_cases as cases
import augment_mask_ref as mref
import augment_ref as ref
from hd_yolo_amd import _lib, augment, build, synth

BG = 0xFFFF


def small_bank(**kw):
    """one 8 x 10 tile, two objects"""
    d = dict(tiles=np.zeros((1, 8, 10, 3), np.uint8), boxes=np.array([[1, 1, 5, 4], [4.5, 3.5, 9.5, 7.5]], np.float32),
             labels=np.array([1, 2], np.int64), offsets=np.array([0, 2], np.int64))
    inst = np.full((1, 8, 10), BG, np.uint16)
    inst[0, 1:4, 1:5] = 0
    inst[0, 3:8, 4:10] = 1                      # later objects overwrite earlier ones: one owner per pixel
    d['instances'] = inst
    d.update(kw)
    return d


def test_tile_bank_validates_the_instance_map(tmp_path):
    ok = small_bank()
    bank = augment.TileBank(**ok)
    assert bank.has_mask.tolist() == [1, 1] and bank.has_mask.dtype == np.uint8 and bank.instances.dtype == np.uint16
    inst = ok['instances']

    def changed(y, x, v):
        m = inst.copy()
        m[0, y, x] = v
        return m

    bad = [dict(instances=inst.astype(np.int32)), dict(instances=inst[:, :7]), dict(instances=inst[0]),
           dict(instances=changed(0, 0, 2)),                       # an object the tile does not have
           dict(instances=changed(1, 0, 0)),                       # left of floor(x1)
           dict(instances=changed(1, 5, 0)),                       # at ceil(x2)
           dict(instances=changed(4, 2, 0)),                       # at ceil(y2)
           dict(instances=changed(2, 6, 1))]                       # above floor(y1) of object 1
    for kw in bad:
        with pytest.raises(ValueError):
            augment.TileBank(**{**ok, **kw})
    edge = augment.TileBank(**{**ok, 'instances': changed(3, 9, 1)})          # x = 9 < ceil(9.5): the box grown to pixel edges
    assert edge.has_mask.tolist() == [1, 1]
    none = augment.TileBank(**{**ok, 'instances': np.full_like(inst, BG)})
    assert none.has_mask.tolist() == [0, 0]
    plain = augment.TileBank(**{k: v for k, v in ok.items() if k != 'instances'})
    assert plain.instances is None and plain.has_mask is None
    # at most 65 535 boxes per tile with a map (0xFFFF is background); without one the limit stays 65 536
    many = dict(tiles=np.zeros((1, 4, 4, 3), np.uint8), boxes=np.zeros((65536, 4), np.float32), labels=np.ones(65536, np.int64),
                offsets=np.array([0, 65536], np.int64))
    augment.TileBank(**many)
    with pytest.raises(ValueError, match='65535'):
        augment.TileBank(**many, instances=np.full((1, 4, 4), BG, np.uint16))
    # save / load
    path = str(tmp_path / 'bank.npz')
    bank.save(path)
    back = augment.TileBank.load(path)
    assert np.array_equal(back.instances, bank.instances) and back.instances.dtype == np.uint16 and np.array_equal(back.has_mask, bank.has_mask)
    assert np.array_equal(back.boxes, bank.boxes) and np.array_equal(back.tiles, bank.tiles)
    plain.save(path)
    assert augment.TileBank.load(path).instances is None
    np.savez(str(tmp_path / 'masks.npz'), masks=np.zeros((2, 28, 28)), **ok)
    with pytest.raises(ValueError, match='masks'):
        augment.TileBank.load(str(tmp_path / 'masks.npz'))


def test_synth_tile_bank_instances_leave_the_other_arrays_bit_identical():
    a = synth.synth_tile_bank(3, 72, 3, seed=5, nmin=6, nmax=12)
    b = synth.synth_tile_bank(3, 72, 3, seed=5, nmin=6, nmax=12, instances=True)
    assert a.instances is None and b.instances.shape == (3, 72, 72) and b.instances.dtype == np.uint16
    for key in ('tiles', 'boxes', 'labels', 'offsets'):
        assert np.array_equal(getattr(a, key), getattr(b, key)) and getattr(a, key).dtype == getattr(b, key).dtype, key
    # every pixel of the map is consistent with its box (TileBank checked it; restated here)
    owned = 0
    for t in range(b.n):
        ys, xs = np.nonzero(b.instances[t] != BG)
        v = b.instances[t][ys, xs].astype(np.int64)
        assert (v < b.offsets[t + 1] - b.offsets[t]).all()
        bx = b.boxes[b.offsets[t] + v]
        assert ((np.floor(bx[:, 0]) <= xs) & (xs < np.ceil(bx[:, 2])) & (np.floor(bx[:, 1]) <= ys) & (ys < np.ceil(bx[:, 3]))).all()
        owned += len(v)
    assert owned > 0.1 * b.instances.size and b.has_mask.sum() >= 0.9 * len(b.boxes)


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


FAKE = 0x10000      # a 16-byte aligned non-NULL "device pointer": the calls below must fail validation before anything dereferences or launches
N_CELLS, PITCH = 8, 5
WS = N_CELLS * PITCH * 32


# the header's parameter lists, in order, with arguments that pass every check
DEFAULTS = {
    'hdy_augment_mask_extents': dict(
        instances=FAKE, n=3, H=40, W=56, bank_boxes=FAKE, has_mask=FAKE, offsets=FAKE, M=9, cells=FAKE, n_cells=N_CELLS, crop=FAKE, B=2, patch=48,
        k=2, img_size=64, ws=FAKE, ws_bytes=WS, pitch=PITCH, stream=None),
    'hdy_augment_boxes_masks': dict(
        bank_boxes=FAKE, bank_labels=FAKE, has_mask=FAKE, offsets=FAKE, n=3, M=9, cells=FAKE, n_cells=N_CELLS, crop=FAKE, B=2, patch=48, k=2,
        img_size=64, ws=FAKE, ws_bytes=WS, pitch=PITCH, out_boxes=FAKE, out_labels=FAKE, out_img=FAKE, out_ref=FAKE, cap=16, counts=FAKE,
        n_counts=2, overflow=FAKE, total=FAKE, stream=None),
    'hdy_augment_mask_targets': dict(
        instances=FAKE, n=3, H=40, W=56, has_mask=FAKE, offsets=FAKE, M=9, cells=FAKE, n_cells=N_CELLS, crop=FAKE, B=2, patch=48, k=2, img_size=64,
        ws=FAKE, ws_bytes=WS, pitch=PITCH, out_boxes=FAKE, out_ref=FAKE, total=FAKE, cap=16, out_masks=FAKE, out_elems=16 * 28 * 28, stream=None),
}


def test_the_argument_lists_below_are_the_headers(lib):
    import re
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'hdyolo.h')).read(), flags=re.S)
    for name, args in DEFAULTS.items():
        params = re.search(name + r'\s*\(([^;]*?)\)\s*;', text, flags=re.S).group(1)
        assert [re.findall(r'(\w+)\s*$', q.strip())[0] for q in params.split(',')] == list(args), name
        assert len(_lib.SIGNATURES[name][1]) == len(args)


@pytest.mark.parametrize('name', sorted(DEFAULTS))
def test_invalid_arguments_return_einval_before_any_launch(lib, name):
    def call(lib, **kw):
        assert set(kw) <= set(DEFAULTS[name])
        return getattr(lib, name)(*{**DEFAULTS[name], **kw}.values())

    extents, boxes_masks, targets = (name.endswith(key) for key in ('mask_extents', 'boxes_masks', 'mask_targets'))
    pointers = [key for key, v in DEFAULTS[name].items() if v == FAKE]
    assert len(pointers) >= 7
    for key in pointers:
        assert call(lib, **{key: None}) == _lib.EINVAL and b'null' in lib.hdy_last_error(), key
    assert call(lib, ws_bytes=WS - 1) == _lib.EINVAL and b'workspace' in lib.hdy_last_error()
    assert call(lib, pitch=PITCH + 1) == _lib.EINVAL and b'workspace' in lib.hdy_last_error()
    assert call(lib, pitch=0) == _lib.EINVAL and call(lib, pitch=65536, ws_bytes=1 << 40) == _lib.EINVAL
    assert call(lib, ws=FAKE + 8) == _lib.EINVAL and b'aligned' in lib.hdy_last_error()
    assert call(lib, cells=FAKE + 2) == _lib.EINVAL and b'aligned' in lib.hdy_last_error()
    assert call(lib, n_cells=N_CELLS + 1, ws_bytes=1 << 20) == _lib.EINVAL and b'cells' in lib.hdy_last_error()
    assert call(lib, k=9) == _lib.EINVAL and call(lib, patch=3) == _lib.EINVAL and call(lib, img_size=97) == _lib.EINVAL
    if not boxes_masks:
        assert call(lib, instances=FAKE + 1) == _lib.EINVAL and b'aligned' in lib.hdy_last_error()
        assert call(lib, H=0) == _lib.EINVAL and call(lib, W=1 << 16) == _lib.EINVAL and call(lib, n=0) == _lib.EINVAL
    if extents:
        assert call(lib, bank_boxes=FAKE + 4) == _lib.EINVAL and b'aligned' in lib.hdy_last_error()
    if boxes_masks:
        assert call(lib, out_boxes=FAKE + 4) == _lib.EINVAL and b'aligned' in lib.hdy_last_error()
        assert call(lib, out_ref=FAKE + 2) == _lib.EINVAL and b'aligned' in lib.hdy_last_error()
        assert call(lib, cap=0) == _lib.EINVAL and call(lib, n_counts=3) == _lib.EINVAL
        assert call(lib, B=2048, k=2, n_cells=8192, ws_bytes=1 << 30) == _lib.EINVAL and b'4096' in lib.hdy_last_error()
    if targets:
        assert call(lib, out_elems=16 * 28 * 28 - 1) == _lib.EINVAL and b'out_masks holds' in lib.hdy_last_error()
        assert call(lib, out_elems=16 * 28 * 28 + 1) == _lib.EINVAL
        assert call(lib, out_masks=FAKE + 4) == _lib.EINVAL and b'aligned' in lib.hdy_last_error()
        assert call(lib, cap=0, out_elems=0) == _lib.EINVAL


# ------------------------------------------------------------------------------------------------------------ the restatement on its own
# Largest |restatement - F.interpolate| over the masked rows of identity_bank() on the CPU: 9.54e-07 (one fp32 rounding of a value near 1:
# torch evaluates the same half-pixel bilinear formula in another order).  The assertion allows four times that.
IDENTITY_MEASURED = 9.54e-07


def identity_bank():
    return synth.synth_tile_bank(3, 64, 2, seed=4, nmin=5, nmax=9, instances=True)


def test_identity_parameters_give_pixel_extents_and_the_bilinear_resize_of_the_crop():
    bank = identity_bank()
    p = augment.identity_params(3, 1, 64, 64)
    p['src'] = np.arange(3).reshape(3, 1)
    tab = augment.cell_tables(p, (64, 64))
    rec, written, rows = mref.augment_masks_ref(bank, tab.cells, tab.crop, 64, 1, 64)
    worst, checked = 0.0, 0
    for t in range(len(rows['boxes'])):
        ci, w = (int(v) for v in rows['ref'][t])
        assert rows['masked'][t] == bool(bank.has_mask[bank.offsets[ci] + w])
        if not rows['masked'][t]:
            assert not rows['masks'][t].any()
            continue
        m = bank.instances[ci] == w                               # the canvas is the tile
        ys, xs = np.nonzero(m)
        assert rec[ci, w, :6].tolist() == [len(xs), xs.min(), xs.max(), ys.min(), ys.max(), len(xs)]
        assert np.array_equal(rows['boxes'][t], np.array([xs.min(), ys.min(), xs.max() + 1, ys.max() + 1], np.float32) / np.float32(64))
        if len(xs) < 25:
            assert not rows['masks'][t].any()
            continue
        crop = torch.from_numpy(m[ys.min():ys.max() + 1, xs.min():xs.max() + 1].astype(np.float32))
        want = F.interpolate(crop[None, None], (28, 28), mode='bilinear', align_corners=False)[0, 0].numpy()
        worst = max(worst, float(np.abs(want - rows['masks'][t]).max()))
        assert rows['masks'][t].min() >= 0 and rows['masks'][t].max() <= 1
        checked += 1
    print(f'identity: {checked} masked rows, largest |restatement - F.interpolate| = {worst:.3e}')
    assert checked >= 10
    assert worst <= 4 * IDENTITY_MEASURED


def test_flips_of_the_restatement_flip_the_image_space_masks():
    """the same parameters with each of the eight flip combinations: every image-space mask is the flipped / transposed unflipped one, the
    extents records follow, and the pixel counts do not change (k = 1 and img_size == patch: the image is the canvas)"""
    bank = cases.hand_bank()
    Bn, P = bank.n, 48
    hyp = cases.make_hyp(1, P, P, 0.001, degrees=30.0, shear=8.0, scale=0.3)
    p = augment.draw_params(np.random.default_rng(3), hyp, Bn, bank.n)
    p['src'] = np.arange(Bn).reshape(Bn, 1)
    p['crop'][:] = 0
    base = None
    for combo in range(8):
        p['hflip'][:], p['vflip'][:], p['transpose'][:] = bool(combo & 1), bool(combo & 2), bool(combo & 4)
        tab = augment.cell_tables(p, (cases.H, cases.W))
        cell, owner = mref.image_owner(bank.instances, tab.cells, tab.crop, P, 1, P)
        rec, _ = mref.mask_extents_ref(bank.instances, bank.has_mask, bank.offsets, len(bank.boxes), tab.cells, tab.crop, P, 1, P, bank.max_per_tile)
        if base is None:
            base, base_rec = owner, rec
            assert (owner != BG).mean() > 0.1
            continue
        want = base
        if combo & 1:
            want = want[:, :, ::-1]
        if combo & 2:
            want = want[:, ::-1, :]
        if combo & 4:
            want = want.transpose(0, 2, 1)
        assert np.array_equal(owner, want), combo
        assert np.array_equal(rec, base_rec), 'records are in pre-flip canvas coordinates; with the whole canvas in the image the area is the count'
        assert np.array_equal(rec[..., 0], rec[..., 5])
        for b in range(Bn):                                       # the forward map (records' area) and the inverse map (image masks) agree
            for w in range(int(bank.offsets[b + 1] - bank.offsets[b])):
                assert int(mref.image_mask(cell, owner, b, b, w).sum()) == int(rec[b, w, 0]) * int(bank.has_mask[bank.offsets[b] + w])


def test_a_map_without_objects_gives_the_boxes_of_the_plain_restatement_bit_for_bit():
    for name in cases.PARITY_CASES:
        case = cases.parity_case(name)
        full, tab = case['bank'], case['tab']
        bank = augment.TileBank(full.tiles, full.boxes, full.labels, full.offsets, np.full_like(full.instances, BG))
        assert not bank.has_mask.any()
        rec, written, rows = mref.augment_masks_ref(bank, tab.cells, tab.crop, cases.PATCH, cases.K, cases.SIZE)
        wb, wl, wi, wc = ref.augment_boxes_ref(bank.boxes, bank.labels, bank.offsets, tab.cells, tab.crop, cases.PATCH, cases.K, cases.SIZE)
        assert len(wb) > 0 and not rec.any() and written.any()
        assert np.array_equal(rows['boxes'].view(np.int32), wb.view(np.int32)) and np.array_equal(rows['labels'], wl)
        assert np.array_equal(rows['img'], wi) and np.array_equal(rows['counts'], wc)
        assert not rows['masks'].any() and not rows['masked'].any()


def test_the_parity_cases_are_not_vacuous():
    """the counts tests/test_gpu_augment_masks.py relies on, from the restatement alone (the seeds of augment_mask_cases.SEEDS were chosen for
    them).  The crop's filter evaluates the UNCLIPPED box behind a candidate test that demands more than 2 pixels, so it can drop nothing
    (include/hdyolo.h says so of hdy_augment_boxes): the filters that can drop a row are the candidate test and the final one."""
    tot = cases.total_stats()
    print(tot)
    assert tot['nonzero_targets'] >= 20 and tot['zeroed_by_25'] >= 1 and tot['unmasked_kept'] >= 1 and tot['kept_at_001_not_010'] >= 1
    assert tot['drop_candidate'] >= 1 and tot['drop_final'] >= 1 and tot['drop_crop'] == 0
    flags = np.concatenate([ref.parse_cells(cases.parity_case(n)['tab'].cells)['flags'] for n in cases.PARITY_CASES])
    assert {int(f) & 7 for f in flags} == set(range(8)) and any(int(f) & 16 for f in flags) and not all(int(f) & 16 for f in flags)
    sizes = np.diff(cases.hand_bank().offsets)
    assert sizes.min() >= 2 and sizes.max() <= 6
