"""Host side of the device augmentation, no GPU: the CPU restatement (tests/augment_ref.py) against goldens made by the reference's own
code (tests/golden/make_golden_augment.py -> augment.npz), known-answer cases, the parameter draw, the packed tables, the tile bank file
format and the argument checks of the two entry points."""
import ctypes
import os

import numpy as np
import pytest

import augment_ref as ref
from hd_yolo_amd import _lib, augment, build, synth

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, 'golden', 'augment.npz'))
NAMES = [str(n) for n in GOLD['names']]
PAR_KEYS = ('c_x', 'c_y', 'p_x', 'p_y', 'angle', 'scale', 'shear_x', 'shear_y', 't_x', 't_y')


def golden_case(name):
    tile, patch, k, S, per_cell = (int(v) for v in GOLD[f'{name}/shape'])
    g = {key: GOLD[f'{name}/{key}'] for key in ('crop', 'boxes', 'src_labels', 'flips', 'pars', 'M', 'pix', 'final', 'labels')}
    g.update(tile=tile, patch=patch, k=k, S=S, per_cell=per_cell)
    g['canvas'] = [(GOLD[f'{name}/canvas_boxes/{j}'], GOLD[f'{name}/canvas_labels/{j}']) for j in range(k * k)]
    return g


def run_golden(g, dt, M=None):
    """every cell of a golden case through the restatement in arithmetic dt -> (pix (T, 4), labels (T,), per-cell (canvas, candidate mask))"""
    k, P, S = g['k'], g['patch'], g['S']
    pix, labels, cells = [], [], []
    for j in range(k * k):
        Mj = g['M'][j] if M is None else M[j]
        flags = int(g['flips'][j][0]) * ref.F_HFLIP + int(g['flips'][j][1]) * ref.F_VFLIP + int(g['flips'][j][2]) * ref.F_TRANSPOSE
        flags += ref.F_PERSP if g['M'][j][2, :2].any() else 0
        Mdt = Mj.astype(dt).reshape(9)
        _, keep, canvas, px = ref.warp_box(g['boxes'][j], Mdt, dt(g['pars'][j][5]), flags, j // k, j % k, P, S, int(g['crop'][0]), int(g['crop'][1]), dt)
        pix.append(px[keep])
        labels.append(g['src_labels'][j][keep])
        cells.append((canvas, px, keep))
    return np.concatenate(pix), np.concatenate(labels), cells


@pytest.mark.parametrize('name', NAMES)
def test_float64_restatement_reproduces_the_reference(name):
    """The goldens are the reference's own estimate_matrix / warp_coords / Mask / box_candidates / *_annotation flips / pad_annotation /
    crop_annotation / remove_invalid_objects / target_to_tensors (cv2.getRotationMatrix2D and skimage.util.crop are restatements in the
    generator: OpenCV's documented formula, array slicing).  Same keep / drop decisions in the same order; coordinates to the last bit where
    the operations are the same (the flips, offsets, clips: exact given equal inputs) and within 1e-9 relative behind the 3 x 3 products,
    which the reference hands to BLAS (`xy @ M.T`, `T @ A @ P @ C`) in an order it does not state."""
    g = golden_case(name)
    pix, labels, cells = run_golden(g, np.float64)
    assert labels.tolist() == g['labels'].tolist(), 'keep / drop decisions and order'
    np.testing.assert_allclose(pix, g['pix'], rtol=1e-9, atol=1e-9 * g['k'] * g['patch'])
    # the canvas boxes of the candidates random_projective kept, cell by cell
    for j, (canvas, _, _) in enumerate(cells):
        gb, gl = g['canvas'][j]
        sel = np.isin(g['src_labels'][j], gl)
        np.testing.assert_allclose(canvas[sel], gb, rtol=1e-9, atol=1e-9 * g['patch'])
    # target_to_tensors: cast to fp32, then divide by the size in fp32
    mine = pix.astype(np.float32) / np.float32(g['S'])
    np.testing.assert_allclose(mine, g['final'], rtol=2.5e-7, atol=0)
    assert (mine == g['final']).mean() > 0.9
    # the matrix composition of hd_yolo_amd.augment from the reference's drawn parameters
    p = {key: g['pars'][:, i] for i, key in enumerate(PAR_KEYS)}
    M = augment.compose_matrices(p, (g['tile'], g['tile']))
    np.testing.assert_allclose(M, g['M'], rtol=1e-9, atol=1e-12)
    pix2, labels2, _ = run_golden(g, np.float64, M=M)
    assert labels2.tolist() == g['labels'].tolist()


@pytest.mark.parametrize('name', NAMES)
def test_fp32_restatement_against_the_float64_goldens(name):
    """The kernel's arithmetic (fp32, every operation rounded on its own) against the reference's float64 result: identical keep / drop
    decisions (the generator keeps every box 0.01 px away from the size thresholds and 1e-3 from the ratio thresholds) and coordinates
    within the bound that follows from the operation chain, u = 2^-24, L = k * patch, A = |x M0| + |y M1| + |M2| <= 4 L (asserted below):
      a corner coordinate X = (x M0 + y M1) + M2 carries the rounding of three matrix entries, two products and two sums: <= 7 u A = 28 u L;
      with the perspective divide (|W| >= 1/2, A_w <= 2, and only |X / W| <= L survives the clip): 2 * 28 u L + 28 u L + u L = 85 u L;
      a flip |x - patch| and the mosaic / crop offset add one rounding of at most u L each: 87 u L in all (1.0e-3 px at L = 192).
    Measured on the four cases: 6.4e-6, 5.3e-6, 1.4e-5 and 8.9e-6 px."""
    g = golden_case(name)
    L, u = g['k'] * g['patch'], 2.0 ** -24
    for j in range(g['k'] * g['k']):
        M, b = np.abs(g['M'][j]), np.abs(g['boxes'][j]).max()
        assert (b * M[:2, 0] + b * M[:2, 1] + M[:2, 2]).max() <= 4 * L and b * M[2, 0] + b * M[2, 1] + 1 <= 2
    pix, labels, _ = run_golden(g, np.float32)
    assert pix.dtype == np.float32
    assert labels.tolist() == g['labels'].tolist(), 'keep / drop decisions and order'
    err = np.abs(pix.astype(np.float64) - g['pix']).max()
    print(f'{name}: fp32 against float64, max |difference| = {err:.3g} px (bound {87 * u * L:.3g})')
    assert err <= 87 * u * L


# ---------------------------------------------------------------------------------------------------------------------- known answers
def tiny_bank(n=3, tile=32, seed=0):
    return synth.synth_tile_bank(n, tile, 2, seed=seed, nmin=3, nmax=5)


def image_of(bank, p, patch, k, S, cval=7):
    tab = augment.cell_tables(p, (bank.H, bank.W))
    return ref.augment_tiles_ref(bank.tiles, tab.cells, tab.crop, patch, k, S, cval), tab


def boxes_of(bank, tab, patch, k, S):
    b, l, i, c = ref.augment_boxes_ref(bank.boxes, bank.labels, bank.offsets, tab.cells, tab.crop, patch, k, S)
    return b * np.float32(S), l, c


def test_identity_parameters_give_the_tile_and_its_boxes():
    bank = tiny_bank()
    p = augment.identity_params(1, 1, 32, 32, src=2)
    img, tab = image_of(bank, p, 32, 1, 32)
    assert np.array_equal(tab.M[0, 0], np.eye(3))
    assert np.array_equal(img[0].transpose(1, 2, 0), bank.tiles[2])
    b, l, c = boxes_of(bank, tab, 32, 1, 32)
    lo, hi = bank.offsets[2], bank.offsets[3]
    big = (bank.boxes[lo:hi, 2] - bank.boxes[lo:hi, 0] > 10) & (bank.boxes[lo:hi, 3] - bank.boxes[lo:hi, 1] > 10)
    assert big.any() and np.allclose(b, bank.boxes[lo:hi][big], atol=1e-5, rtol=0) and l.tolist() == bank.labels[lo:hi][big].tolist()


@pytest.mark.parametrize('flip', ['hflip', 'vflip', 'transpose'])
def test_pure_flips_reverse_or_transpose_the_tile(flip):
    bank = tiny_bank()
    p = augment.identity_params(1, 1, 32, 32, src=1)
    p[flip][:] = True
    img, tab = image_of(bank, p, 32, 1, 32)
    t = bank.tiles[1]
    want = {'hflip': t[:, ::-1], 'vflip': t[::-1], 'transpose': t.swapaxes(0, 1)}[flip]
    assert np.array_equal(img[0].transpose(1, 2, 0), want)
    b, _, _ = boxes_of(bank, tab, 32, 1, 32)
    src = bank.boxes[bank.offsets[1]:bank.offsets[2]]
    src = src[(src[:, 2] - src[:, 0] > 10) & (src[:, 3] - src[:, 1] > 10)]
    wantb = {'hflip': np.stack([32 - src[:, 2], src[:, 1], 32 - src[:, 0], src[:, 3]], 1),
             'vflip': np.stack([src[:, 0], 32 - src[:, 3], src[:, 2], 32 - src[:, 1]], 1), 'transpose': src[:, [1, 0, 3, 2]]}[flip]
    assert np.allclose(b, wantb, atol=1e-5, rtol=0)


def test_source_entirely_outside_gives_the_border_value_and_drops_its_boxes():
    bank = tiny_bank()
    p = augment.identity_params(1, 1, 32, 32, src=0)
    p['t_x'][:] = 16 + 200.0                                     # the tile lands 200 px to the right of the canvas
    img, tab = image_of(bank, p, 32, 1, 32, cval=201)
    assert (img == 201).all()
    b, l, c = boxes_of(bank, tab, 32, 1, 32)
    # documented rule: the clipped corners all sit on x = patch: zero width, box_candidates (w2 > 2) drops the box
    assert len(b) == 0 and c.tolist() == [0]
    p['t_x'][:] = 16 - 200.0                                     # ... and to the left: every clipped x is 0, Mask.box gives the zero box
    _, tab = image_of(bank, p, 32, 1, 32)
    assert boxes_of(bank, tab, 32, 1, 32)[2].tolist() == [0]


def test_half_pixel_shift_interpolates_with_the_stated_integer_weights():
    bank = tiny_bank()
    p = augment.identity_params(1, 1, 32, 32, src=0)
    p['t_x'][:] = 16 - 0.5                                       # canvas x reads source x + 1/2: fx = 16
    img, _ = image_of(bank, p, 32, 1, 32, cval=0)
    t = bank.tiles[0].astype(np.int64)
    want = (t[:, :-1] * 512 + t[:, 1:] * 512 + 512) >> 10
    assert np.array_equal(img[0].transpose(1, 2, 0)[:, :-1], want)
    assert np.array_equal(img[0].transpose(1, 2, 0)[:, -1], (t[:, -1] * 512 + 512) >> 10)       # the last column mixes with the border (0)


def test_hsv_round_trip_known_values():
    ident = np.tile(np.arange(256, dtype=np.uint8), (3, 1))
    ident[0] = np.arange(256) % 180
    grey = np.arange(256)
    r, g, b = ref.hsv_round_trip(grey, grey, grey, np.broadcast_to(ident, (256, 3, 256)))
    assert np.array_equal(r, grey) and np.array_equal(g, grey) and np.array_equal(b, grey), 'greys have no hue or saturation'
    prim = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255]])
    out = np.stack(ref.hsv_round_trip(prim[:, 0], prim[:, 1], prim[:, 2], np.broadcast_to(ident, (6, 3, 256))), 1)
    assert np.array_equal(out, prim), 'primaries and secondaries sit on sector borders: H = 0, 60, 120, 30, 90, 150'
    rng = np.random.default_rng(0)
    px = rng.integers(0, 256, (4096, 3))
    out = np.stack(ref.hsv_round_trip(px[:, 0], px[:, 1], px[:, 2], np.broadcast_to(ident, (4096, 3, 256))), 1)
    assert np.abs(out - px).max() <= 5, '8-bit HSV is lossy (180 hues), but an identity table stays close'
    # a value table of zeros gives black, a saturation table of zeros gives the grey of V
    dark = ident.copy()
    dark[2] = 0
    assert not np.stack(ref.hsv_round_trip(px[:, 0], px[:, 1], px[:, 2], np.broadcast_to(dark, (4096, 3, 256))), 1).any()
    unsat = ident.copy()
    unsat[1] = 0
    out = np.stack(ref.hsv_round_trip(px[:, 0], px[:, 1], px[:, 2], np.broadcast_to(unsat, (4096, 3, 256))), 1)
    assert np.array_equal(out, np.repeat(px.max(1)[:, None], 3, 1))
    # the tables as random_hsv makes them
    lut = augment.hsv_luts(np.array([1.2, 0.5, 1.5]))
    x = np.arange(256, dtype=np.float64)
    assert np.array_equal(lut[0], ((x * 1.2) % 180).astype(np.uint8)) and lut[0].max() < 180
    assert np.array_equal(lut[1], np.clip(x * 0.5, 0, 255).astype(np.uint8)) and lut[2][-1] == 255 and lut[2][100] == 150


def test_crop_filter_looks_at_the_unclipped_box():
    """remove_invalid_objects after the crop clips new_ann but evaluates `x1 < x2 & y1 < y2` on the UNCLIPPED input: a box wholly outside
    the crop window passes that pass (its clipped form is degenerate) and is only removed by the final 10 px filter, which looks at the
    output of the first pass.  Hand-made: a 2 x 1 ... 2 x 2 mosaic of 32 px cells, crop window (32, 0) + 32: cell (0, 0) lies outside."""
    flags, eye = 0, np.eye(3, dtype=np.float32).reshape(9)
    box = np.array([[4, 4, 28, 28]], np.float32)
    res, keep, _, pix = ref.warp_box(box, eye, 1.0, flags, 0, 0, 32, 32, 32, 0, np.float32)
    assert pix.tolist() == [[0, 4, 0, 28]] and not keep[0], 'outside the window: degenerate after the clip, dropped by the final filter'
    # the same box in the cell the window shows: kept, unchanged
    res, keep, _, pix = ref.warp_box(box, eye, 1.0, flags, 0, 1, 32, 32, 32, 0, np.float32)
    assert keep[0] and pix.tolist() == [[4, 4, 28, 28]]
    # a box that straddles the window's edge is clipped, and kept while more than 10 px remain
    wide = np.array([[20, 4, 31, 28]], np.float32)
    _, keep, _, pix = ref.warp_box(wide, eye, 1.0, flags, 0, 0, 32, 64, 25, 0, np.float32)      # window x from 25: 6 px of the box remain
    assert pix.tolist() == [[0, 4, 6, 28]] and not keep[0]
    _, keep, _, pix = ref.warp_box(wide, eye, 1.0, flags, 0, 0, 32, 64, 5, 0, np.float32)
    assert keep[0] and pix.tolist() == [[15, 4, 26, 28]]


# ------------------------------------------------------------------------------------------------------------- parameters and tables
HYP = dict(degrees=10.0, translate=0.1, scale=0.2, shear=5.0, perspective=0.001, hsv_h=0.015, hsv_s=0.7, hsv_v=0.4, fliplr=0.5, flipud=0.3,
           transpose=0.2, cval=0.5, k_mosaic=2, patch_size=64, img_size=96)


def test_draw_is_deterministic_per_seed_rank_epoch_step_and_ranks_differ():
    a = augment.draw_params(augment.step_rng(3, 1, 2, 5), HYP, 4, 10)
    b = augment.draw_params(augment.step_rng(3, 1, 2, 5), HYP, 4, 10)
    assert all(np.array_equal(a[key], b[key]) for key in a)
    for other in ((4, 1, 2, 5), (3, 0, 2, 5), (3, 1, 3, 5), (3, 1, 2, 6)):
        c = augment.draw_params(augment.step_rng(*other), HYP, 4, 10)
        assert not np.array_equal(a['angle'], c['angle']) and not np.array_equal(a['src'], c['src'])
    assert augment.step_seed(3, 1, 2, 5) == 3 + 1000003 + 2 * 7919 + 5, 'the mixing of SyntheticTiles'


def test_draw_supports_match_the_reference_bounds():
    p = augment.draw_params(np.random.default_rng(0), HYP, 512, 7)
    assert p['src'].shape == (512, 4) and p['src'].min() == 0 and p['src'].max() == 6
    for key, lo, hi in (('angle', -10, 10), ('scale', 0.8, 1.2), ('shear_x', -5, 5), ('shear_y', -5, 5), ('p_x', -0.001, 0.001),
                        ('p_y', -0.001, 0.001), ('t_x', 0.4 * 64, 0.6 * 64), ('t_y', 0.4 * 64, 0.6 * 64)):
        v = p[key]
        assert lo <= v.min() < lo + 0.02 * (hi - lo) and hi - 0.02 * (hi - lo) < v.max() <= hi, key
    g = p['hsv_gain']
    assert 1 - 0.015 <= g[..., 0].min() and g[..., 0].max() <= 1.015 and 0.3 <= g[..., 1].min() and g[..., 1].max() <= 1.7 and g[..., 2].max() <= 1.4
    for key, prob in (('hsv', 0.5), ('hflip', 0.5), ('vflip', 0.3), ('transpose', 0.2)):
        assert abs(p[key].mean() - prob) < 0.05, key
    assert p['crop'].min() == 0 and p['crop'].max() == 2 * 64 - 96, 'get_crop_width: randint(0, input - output + 1)'
    none = augment.draw_params(np.random.default_rng(0), dict(HYP, hsv_h=0, hsv_s=0, hsv_v=0, fliplr=0, flipud=0, transpose=0), 64, 7)
    assert not none['hsv'].any() and not none['hflip'].any() and not none['vflip'].any() and not none['transpose'].any()
    for key in augment.HYP_KEYS:
        missing = dict(HYP)
        del missing[key]
        with pytest.raises(KeyError):
            augment.draw_params(np.random.default_rng(0), missing, 2, 7)
    assert augment.border_byte(0.5) == 0 and augment.border_byte(1.5) == 2 and augment.border_byte(114) == 114 and augment.border_byte(300) == 255


def test_packed_tables_hold_what_the_header_states():
    p = augment.draw_params(np.random.default_rng(1), HYP, 3, 5)
    tab = augment.cell_tables(p, (48, 40))
    assert tab.packed.shape == (12 * 864 + 3 * 8,) and tab.cells.shape == (12, 864) and tab.crop.tolist() == p['crop'].tolist()
    c = ref.parse_cells(tab.cells)
    assert c['src'].tolist() == p['src'].reshape(-1).tolist()
    assert np.array_equal(c['M'], tab.M.reshape(12, 9).astype(np.float32)) and np.array_equal(c['Minv'], tab.Minv.reshape(12, 9).astype(np.float32))
    assert np.allclose(tab.M @ tab.Minv, np.eye(3), atol=1e-9)
    want = p['hflip'] * 1 + p['vflip'] * 2 + p['transpose'] * 4 + p['hsv'] * 8 + 16
    assert c['flags'].tolist() == want.reshape(-1).tolist()
    assert np.array_equal(c['scale'], p['scale'].reshape(-1).astype(np.float32))
    assert np.array_equal(c['lut'], augment.hsv_luts(p['hsv_gain']).reshape(12, 3, 256))
    assert not tab.cells[:, 84:96].any()
    # the centre of the source tile lands on (t_x, t_y)
    centre = tab.M.reshape(12, 3, 3) @ np.array([20.0, 24.0, 1.0])
    assert np.allclose(centre[:, :2] / centre[:, 2:], np.stack([p['t_x'].reshape(-1), p['t_y'].reshape(-1)], 1))
    flat = augment.cell_tables(dict(p, p_x=p['p_x'] * 0, p_y=p['p_y'] * 0), (48, 40))
    assert not (ref.parse_cells(flat.cells)['flags'] & 16).any()


def test_tile_bank_round_trip_and_refusals(tmp_path):
    bank = synth.synth_tile_bank(4, 24, 3, seed=2, nmin=2, nmax=4)
    again = synth.synth_tile_bank(4, 24, 3, seed=2, nmin=2, nmax=4)
    assert np.array_equal(bank.tiles, again.tiles) and np.array_equal(bank.boxes, again.boxes), 'seeded'
    assert bank.tiles.dtype == np.uint8 and bank.tiles.shape == (4, 24, 24, 3) and bank.labels.min() >= 1 and bank.labels.max() <= 3
    path = str(tmp_path / 'bank.npz')
    bank.save(path)
    back = augment.TileBank.load(path)
    assert all(np.array_equal(getattr(bank, key), getattr(back, key)) for key in ('tiles', 'boxes', 'labels', 'offsets'))
    assert back.n == 4 and back.H == back.W == 24 and back.max_per_tile == int(np.diff(bank.offsets).max())
    ok = dict(tiles=bank.tiles, boxes=bank.boxes, labels=bank.labels, offsets=bank.offsets)
    bad = [dict(ok, tiles=bank.tiles.astype(np.float32)), dict(ok, tiles=bank.tiles[..., 0]), dict(ok, boxes=bank.boxes.astype(np.float64)),
           dict(ok, labels=bank.labels.astype(np.int32)), dict(ok, offsets=bank.offsets[:-1]), dict(ok, offsets=bank.offsets[::-1].copy()),
           dict(ok, labels=bank.labels * 0), dict(ok, boxes=bank.boxes * np.float32('nan')),
           dict(ok, tiles=np.array([bank.tiles[0], bank.tiles[1][:20]], dtype=object))]
    for kw in bad:
        with pytest.raises(ValueError):
            augment.TileBank(**kw)
    np.savez(str(tmp_path / 'masks.npz'), masks=np.zeros((1, 28, 28)), **ok)
    with pytest.raises(ValueError, match='mask'):
        augment.TileBank.load(str(tmp_path / 'masks.npz'))
    np.savez(str(tmp_path / 'short.npz'), tiles=bank.tiles)
    with pytest.raises(ValueError, match='missing'):
        augment.TileBank.load(str(tmp_path / 'short.npz'))
    for hyp in (dict(HYP, color_aug='jitter'), dict(HYP, keep_res=0.5), dict(HYP, img_size=200), dict(HYP, k_mosaic=0), dict(HYP, patch_size=2)):
        with pytest.raises(ValueError):
            augment.check_hyp(hyp)


# ------------------------------------------------------------------------------------------------------------------------------- ABI
FAKE = 0x10000


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


def test_entry_points_check_sizes_before_anything_is_launched(lib):
    assert _lib.ABI_VERSION >= 9 and augment.CELL_BYTES == 864
    B, k, P, S = 4, 2, 48, 64

    def tiles(out_elems=B * 3 * S * S, n_cells=B * k * k, **kw):
        a = dict(pb=3, n=5, H=40, W=40, patch=P, k=k, S=S, cval=0, dtype=_lib.BF16, pitch=120, stride=4800)
        a.update(kw)
        return lib.hdy_augment_tiles_u8(FAKE, a['stride'], a['pitch'], a['pb'], a['n'], a['H'], a['W'], FAKE, n_cells, FAKE, B, a['patch'], a['k'], a['S'],
                                        a['cval'], FAKE, out_elems, a['dtype'], None)

    for kw, word in ((dict(out_elems=B * 3 * S * S - 1), b'out holds'), (dict(out_elems=B * 4 * S * S), b'out holds'), (dict(n_cells=15), b'cell table'),
                     (dict(pb=2), b'pixel_bytes'), (dict(pitch=119), b'pitch'), (dict(stride=4000), b'tile stride'), (dict(k=9), b'mosaic side'),
                     (dict(S=97), b'img_size'), (dict(patch=3), b'patch'), (dict(cval=256), b'border value'), (dict(dtype=2), b'dtype')):
        assert tiles(**kw) == _lib.EINVAL and word in lib.hdy_last_error(), (kw, lib.hdy_last_error())
    assert lib.hdy_augment_tiles_u8(None, 4800, 120, 3, 5, 40, 40, FAKE, 16, FAKE, B, P, k, S, 0, FAKE, B * 3 * S * S, _lib.BF16, None) == _lib.EINVAL

    def boxes(cap=100, n_cells=B * k * k, n_counts=B, Bk=k, M=50, out=FAKE):
        return lib.hdy_augment_boxes(FAKE, FAKE, FAKE, 5, M, FAKE, n_cells, FAKE, B, P, Bk, S, out, FAKE, FAKE, cap, FAKE, n_counts, FAKE, None)

    for kw, word in ((dict(cap=0), b'capacity'), (dict(cap=-5), b'capacity'), (dict(n_cells=17), b'cell table'), (dict(n_counts=3), b'counts'),
                     (dict(M=-1), b'boxes'), (dict(out=FAKE + 4), b'aligned'), (dict(out=None), b'null')):
        assert boxes(**kw) == _lib.EINVAL and word in lib.hdy_last_error(), (kw, lib.hdy_last_error())
    assert lib.hdy_augment_boxes(FAKE, FAKE, FAKE, 5, 50, FAKE, 1025 * 4, FAKE, 1025, P, 2, S, FAKE, FAKE, FAKE, 10, FAKE, 1025, FAKE, None) == _lib.EINVAL
    assert b'at most 4096' in lib.hdy_last_error()
    assert lib.hdy_exec_op(b'hdy_augment_tiles_u8') >= 0 and lib.hdy_exec_op(b'hdy_augment_boxes') >= 0
    assert isinstance(ctypes.c_void_p(FAKE).value, int)
