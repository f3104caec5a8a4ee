"""CPU tests of the texture pass's specification and surroundings: the numpy restatements of include/hdyolo_texture.h against each other and
against hand-derived cases, the features of hd_yolo_amd/texture.py against their loop restatement, the header and its binding through
_ext.EXTENSIONS, every argument check of hdy_label_texture (reached with fake pointers: nothing launches), and stain_lut over all 2^24 colours."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import texture_ref as ref
from hd_yolo_amd import _header, _lib, build
from hd_yolo_amd import texture as htexture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFFS4 = ((0, 1), (-1, 1), (-1, 0), (-1, -1))
NAN = float('nan')


def _random_case(seed, h=37, w=53, R=7, levels=16):
    rng = np.random.default_rng(seed)
    lm = rng.integers(-1, R + 2, size=(h, w)).astype(np.int32)
    lm[rng.random((h, w)) < 0.05] = 0x7fffffff
    lm[10:30, 5:40][rng.random((20, 35)) < 0.7] = 3                       # one label with real neighbourhoods
    rgb = rng.integers(0, 256, size=(h, w, 3)).astype(np.uint8)
    lut = rng.integers(-(1 << 16) * levels // 6, (1 << 16) * levels // 2, size=(3, 256)).astype(np.int32)
    ext = np.stack([rng.integers(-5, w // 2, R), rng.integers(-5, h // 2, R), rng.integers(w // 2, w + 5, R), rng.integers(h // 2, h + 5, R)], 1)
    ext[1] = (w, h, -1, -1)
    return lm, rgb, ext.astype(np.int32), lut


@pytest.mark.parametrize('seed, levels, offsets', [(0, 16, OFFS4), (1, 8, ((0, 1), (0, -1))), (2, 32, ((4, -4), (-3, 2), (1, 0)))])
def test_the_two_restatements_agree_on_random_maps(seed, levels, offsets):
    lm, rgb, ext, lut = _random_case(seed, levels=levels)
    a = ref.texture_loop(lm, rgb, ext, lut, levels, offsets)
    b = ref.texture_vec(lm, rgb, ext, lut, levels, offsets)
    for x, y in zip(a, b):
        assert x.dtype == np.int32 and np.array_equal(x, y)
    hist, glcm, flags = a
    assert flags[1] == 1 and not hist[1].any() and not glcm[1].any() and hist.sum() > 0 and glcm.sum() > 0
    assert np.array_equal(glcm, glcm.transpose(0, 1, 3, 2)) and (glcm.sum((2, 3)) % 2 == 0).all()       # symmetric, two adds per pair
    # a sub-range of rows is the same rows of the whole call
    part = ref.texture_vec(lm, rgb, ext, lut, levels, offsets, row0=2, rows=3)
    for x, y in zip(part, a):
        assert np.array_equal(x, y[2:5])
    if levels == 8:               # (0, 1) and (0, -1) see the same pairs from their two ends, where the box holds the whole label (the window does)
        whole = np.tile(np.array([[0, 0, lm.shape[1] - 1, lm.shape[0] - 1]], np.int32), (len(ext), 1))
        _, g, _ = ref.texture_vec(lm, rgb, whole, lut, levels, offsets)
        assert np.array_equal(g[:, 0], g[:, 1]) and not np.array_equal(glcm[:, 0], glcm[:, 1])


def _ident_lut(levels):
    """level = R channel value, clamped: entries v << 16 on the first row"""
    lut = np.zeros((3, 256), np.int32)
    lut[0] = np.arange(256) << 16
    return lut


def _features(glcm):
    return htexture.haralick(torch.from_numpy(np.asarray(glcm, dtype=np.int32))[None, None])[0, 0].tolist()


def test_constant_nucleus():
    lm = np.full((6, 9), -1, np.int32)
    lm[1:5, 2:8] = 0                                                      # 4 x 6 entries, all of level 5
    rgb = np.full((6, 9, 3), 5, np.uint8)
    ext = np.array([[2, 1, 7, 4]], np.int32)
    hist, glcm, flags = ref.texture_loop(lm, rgb, ext, _ident_lut(16), 16, OFFS4)
    assert flags.tolist() == [0] and hist[0].tolist() == [0] * 5 + [24] + [0] * 10
    pairs = [4 * 5, 3 * 5, 3 * 6, 3 * 5]                                  # (0, 1), (-1, 1), (-1, 0), (-1, -1) inside a 4 x 6 block
    for d in range(4):
        want = np.zeros((16, 16), np.int32)
        want[5, 5] = 2 * pairs[d]
        assert np.array_equal(glcm[0, d], want)
        f = _features(glcm[0, d])
        assert f[0] == 1 and f[1] == 0 and f[2] == 1 and f[8] == 0 and f[11] == 0 and f[12] == 0 and f[5] == 10 and f[3] == 0
        assert ref.haralick_loop(glcm[0, d]) == f
    stats = htexture.intensity(torch.from_numpy(hist), 16)
    assert [stats[k].item() for k in htexture.INTENSITY] == [5, 0, 0, 0, 0, 5, 5, 5] == ref.intensity_loop(hist[0])


def test_two_level_checkerboard():
    lm = np.zeros((8, 8), np.int32)
    rgb = np.zeros((8, 8, 3), np.uint8)
    rgb[..., 0] = (np.add.outer(np.arange(8), np.arange(8)) & 1) * 3      # levels 0 and 3
    ext = np.array([[0, 0, 7, 7]], np.int32)
    hist, glcm, _ = ref.texture_loop(lm, rgb, ext, _ident_lut(8), 8, ((0, 1), (-1, 1)))
    assert hist[0].tolist() == [32, 0, 0, 32, 0, 0, 0, 0]
    want = np.zeros((8, 8), np.int32)
    want[0, 3] = want[3, 0] = 8 * 7                                       # 56 horizontal pairs, each of levels (0, 3): all mass off the diagonal
    assert np.array_equal(glcm[0, 0], want)
    f = _features(glcm[0, 0])
    assert f[1] == 9 and f[0] == 0.5 and f[2] == -1 and abs(f[8] - math.log(2)) < 1e-15      # contrast (3 - 0)^2, two equal cells
    # with unit level spacing the contrast is 1
    rgb[..., 0] //= 3
    _, g1, _ = ref.texture_loop(lm, rgb, ext, _ident_lut(8), 8, ((0, 1), (-1, 1)))
    assert _features(g1[0, 0])[1] == 1 and np.trace(g1[0, 0]) == 0
    # the diagonal offset pairs equal levels only: all mass on the diagonal
    assert np.trace(glcm[0, 1]) == glcm[0, 1].sum() == 2 * 49 and _features(glcm[0, 1])[1] == 0


def test_single_pixel_has_a_histogram_only():
    lm = np.full((5, 5), -1, np.int32)
    lm[2, 3] = 0
    rgb = np.full((5, 5, 3), 9, np.uint8)
    hist, glcm, flags = ref.texture_loop(lm, rgb, np.array([[3, 2, 3, 2]], np.int32), _ident_lut(16), 16, OFFS4)
    assert flags[0] == 0 and hist[0].sum() == 1 and hist[0, 9] == 1 and not glcm.any()
    f = htexture.haralick(torch.from_numpy(glcm))
    assert f.shape == (1, 4, 13) and bool(torch.isnan(f).all())
    assert all(math.isnan(v) for v in ref.haralick_loop(glcm[0, 0]))
    cols = htexture.columns(torch.from_numpy(hist), torch.from_numpy(glcm), torch.from_numpy(flags))
    assert cols['tex_level_mean'].item() == 9 and math.isnan(cols['tex_contrast_mean'].item()) and math.isnan(cols['tex_entropy_range'].item())
    assert len(cols) == 8 + 26 + 1 and all(v.dtype == torch.float64 and v.shape == (1,) for v in cols.values())


def test_features_equal_their_loop_restatement():
    lm, rgb, ext, lut = _random_case(5)
    hist, glcm, flags = ref.texture_vec(lm, rgb, ext, lut, 16, OFFS4)
    got = htexture.haralick(torch.from_numpy(glcm)).numpy()
    want = np.array([[ref.haralick_loop(glcm[q, d]) for d in range(4)] for q in range(len(ext))])
    got[..., 12], want[..., 12] = got[..., 12] ** 2, want[..., 12] ** 2   # imc2 through its square: the root of a difference near zero
    assert np.isnan(want[1]).all() and np.isfinite(want[3]).all()
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-12, equal_nan=True)
    stats = htexture.intensity(torch.from_numpy(hist), 16)
    got_i = np.stack([stats[k].numpy() for k in htexture.INTENSITY], 1)
    np.testing.assert_allclose(got_i, np.array([ref.intensity_loop(hv) for hv in hist]), rtol=1e-9, atol=1e-12, equal_nan=True)
    # the table's mean and range over the directions that have pairs
    cols = htexture.columns(torch.from_numpy(hist), torch.from_numpy(glcm), torch.from_numpy(flags))
    full = np.array([[ref.haralick_loop(glcm[q, d]) for d in range(4)] for q in range(len(ext))])
    for k, name in enumerate(htexture.FEATURES):
        if name == 'imc2':
            continue
        for q in range(len(ext)):
            vals = [v for v in full[q, :, k] if not math.isnan(v)]
            m, s = (sum(vals) / len(vals), max(vals) - min(vals)) if vals else (NAN, NAN)
            np.testing.assert_allclose(cols[f'tex_{name}_mean'][q].item(), m, rtol=1e-9, atol=1e-12, equal_nan=True)
            np.testing.assert_allclose(cols[f'tex_{name}_range'][q].item(), s, rtol=1e-9, atol=1e-9, equal_nan=True)
    assert cols['tex_flags'].tolist() == flags.tolist()


# ---- the extension header and its binding, through the built library ------------------------------------------------------------------------
FAKE = 0x10000      # an aligned non-NULL "device pointer": every call below must fail validation before anything dereferences or launches


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    from hd_yolo_amd import _ext
    return _ext.load()


def test_texture_header_parses_and_is_bound_beside_the_four(lib):
    from hd_yolo_amd import _ext
    path = os.path.join(ROOT, 'include', 'hdyolo_texture.h')
    assert _header.EXTENSION_NAMES[-1] == 'texture' and list(_ext.EXTENSIONS)[-1] == 'texture'
    ext = _ext.EXTENSIONS['texture']
    assert ext.header == path == _header.extension_header('texture')
    hdr = _header.read(path)
    assert sorted(hdr.functions) == ['hdy_label_texture', 'hdy_texture_revision'] and not hdr.structs
    assert hdr.constants == {'HDY_TEXTURE_REVISION': 1, 'HDY_TEXTURE_MAX_SIDE': 1024, 'HDY_TEXTURE_MAX_WINDOW': 1 << 29, 'HDY_TEXTURE_SHIFT': 16,
                             'HDY_TEXTURE_MAX_LEVELS': 32, 'HDY_TEXTURE_MAX_OFFSETS': 4, 'HDY_TEXTURE_MAX_REACH': 4}
    res, args = hdr.functions['hdy_label_texture']
    vp, ll, i = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int
    assert res is i and args == [vp, ll, i, i, vp, ll, ll, i, i, i, vp, ll, i, vp, ll, i, vp, ll, i, i, i, vp, ll, vp, ll, vp, ll, vp]
    assert [p[0] for p in hdr.params['hdy_label_texture']][10:21] == ['extent', 'extent_elems', 'R', 'lut', 'lut_elems', 'levels', 'offsets',
                                                                     'offsets_elems', 'D', 'row0', 'rows']
    for name, (res, args) in hdr.functions.items():
        fn = getattr(lib, name)                                            # exported by the built library ...
        assert fn.restype is res and list(fn.argtypes) == args, name      # ... and bound by _ext.load()
        assert name not in _lib.SIGNATURES                                 # the numbered ABI does not know the extension
        assert _ext.SIGNATURES[name] == (res, args) and _ext.PARAMS[name] == hdr.params[name]
    assert (ext.functions, ext.params, ext.constants) == (hdr.functions, hdr.params, hdr.constants)
    assert (ext.revision_fn, ext.revision_macro) == ('hdy_texture_revision', 'HDY_TEXTURE_REVISION')
    assert lib.hdy_texture_revision() == ext.revision == 1
    assert ext.constants['HDY_TEXTURE_SHIFT'] == htexture.SHIFT == ref.SHIFT and ext.constants['HDY_TEXTURE_MAX_SIDE'] == ref.MAX_SIDE
    assert not any(k.startswith('HDY_TEXTURE') for k in _lib.CONSTANTS)
    assert {k: v for k, v in _ext.CONSTANTS.items() if k.startswith('HDY_TEXTURE')} == hdr.constants and len(hdr.constants) == 7
    # one list: five headers, 15 functions, 22 constants
    assert list(_ext.EXTENSIONS) == ['measure', 'spatial', 'outline', 'graph', 'texture'] == list(_header.EXTENSION_NAMES)
    assert len(_ext.SIGNATURES) == 15 and len(_ext.PARAMS) == 15 and len(_ext.CONSTANTS) == 22
    assert 'texture.hip' in build.SOURCES


def test_a_name_belongs_to_one_header_across_both_lists():
    from hd_yolo_amd import _ext
    both = dict(_ext.EXTENSIONS)                                          # one table now: the five headers
    _ext.check_disjoint(both)                                             # the tables as they are pass
    tex = both['texture']
    doctored = tex._replace(functions=dict(tex.functions, hdy_label_measure=_ext.SIGNATURES['hdy_label_measure']))
    with pytest.raises(_lib.HdyError) as e:
        _ext.check_disjoint(dict(both, texture=doctored))
    assert 'hdy_label_measure is declared by include/hdyolo_measure.h and by include/hdyolo_texture.h' in str(e.value)
    with pytest.raises(_lib.HdyError) as e:
        _ext.check_disjoint(dict(both, texture=tex._replace(constants=dict(tex.constants, HDY_ABI_VERSION=1))))
    assert 'HDY_ABI_VERSION is declared by include/hdyolo.h and by include/hdyolo_texture.h' in str(e.value)
    assert 'hdy_label_measure' not in tex.functions


def _call(lib, **kw):
    """hdy_label_texture on a 20 x 30 window of a 100-byte-pitch RGB image, 5 labels, 16 levels, 2 offsets, rows 1 .. 3"""
    a = dict(map=FAKE, map_elems=20 * 30, h=20, w=30, image=FAKE + 1, image_bytes=19 * 100 + 29 * 3 + 3, row_stride=100, pixel_stride=3, x0=0, y0=0,
             extent=FAKE, extent_elems=20, R=5, lut=FAKE, lut_elems=768, levels=16, offsets=[0, 1, -1, 0], offsets_elems=4, D=2, row0=1, rows=3,
             hist=FAKE, hist_elems=3 * 16, glcm=FAKE, glcm_elems=3 * 2 * 256, flags=FAKE, flags_elems=3)
    a.update(kw)
    offs = a['offsets']
    if isinstance(offs, list):
        offs = (ctypes.c_int * max(len(offs), 1))(*offs)
    rc = lib.hdy_label_texture(a['map'], a['map_elems'], a['h'], a['w'], a['image'], a['image_bytes'], a['row_stride'], a['pixel_stride'], a['x0'],
                               a['y0'], a['extent'], a['extent_elems'], a['R'], a['lut'], a['lut_elems'], a['levels'], offs, a['offsets_elems'],
                               a['D'], a['row0'], a['rows'], a['hist'], a['hist_elems'], a['glcm'], a['glcm_elems'], a['flags'], a['flags_elems'],
                               None)
    return rc, lib.hdy_last_error()


def test_label_texture_argument_checks(lib):
    for name in ('map', 'image', 'extent', 'lut', 'offsets', 'hist', 'glcm', 'flags'):
        rc, msg = _call(lib, **{name: None})
        assert rc == _lib.EINVAL and b'null' in msg and name.encode() in msg, name
    for name in ('map', 'extent', 'lut', 'hist', 'glcm', 'flags'):
        rc, msg = _call(lib, **{name: FAKE + 2})
        assert rc == _lib.EINVAL and b'misaligned' in msg and name.encode() in msg, name
    holder = (ctypes.c_int * 6)(0, 0, 1, -1, 0, 0)
    rc, msg = _call(lib, offsets=ctypes.c_void_p(ctypes.addressof(holder) + 2))
    assert rc == _lib.EINVAL and b'misaligned' in msg and b'offsets' in msg
    for kw in ({'R': -1, 'extent_elems': -4}, {'map_elems': -600}, {'extent_elems': -1}, {'lut_elems': -768}, {'offsets_elems': -4},
               {'hist_elems': -1}, {'glcm_elems': -1}, {'flags_elems': -3}):
        rc, msg = _call(lib, **kw)
        assert rc == _lib.EINVAL and b'negative' in msg and list(kw)[-1].encode() in msg, kw
    for kw in ({'h': 0, 'map_elems': 0}, {'w': -5}, {'h': (1 << 29) + 1, 'w': 1, 'map_elems': (1 << 29) + 1}):
        rc, msg = _call(lib, **kw)
        assert rc == _lib.EINVAL and b'outside [1, 536870912]' in msg, kw
    for name, good in (('map_elems', 600), ('extent_elems', 20), ('lut_elems', 768), ('offsets_elems', 4), ('hist_elems', 48),
                       ('glcm_elems', 1536), ('flags_elems', 3)):
        for n in (good - 1, good + 1, 0):
            rc, msg = _call(lib, **{name: n})
            assert rc == _lib.EINVAL and name.encode() in msg, (name, n)
    # 64-bit sizes: the count that 32-bit arithmetic would give for a 70 000 x 70 000 window is refused
    rc, msg = _call(lib, h=70000, w=70000, map_elems=(70000 * 70000) & 0xFFFFFFFF)
    assert rc == _lib.EINVAL and b'map_elems' in msg
    for lv in (0, 4, 12, 17, 64, -16):
        rc, msg = _call(lib, levels=lv)
        assert rc == _lib.EINVAL and b'levels' in msg, lv
    for D in (0, 5, -1):
        rc, msg = _call(lib, D=D, offsets_elems=2 * max(D, 0), offsets=[0, 1] * 5)
        assert rc == _lib.EINVAL and b'D=' in msg, D
    for bad in ([0, 1, 5, 0], [0, 1, 0, -5], [-5, 1, 1, 0]):
        rc, msg = _call(lib, offsets=bad)
        assert rc == _lib.EINVAL and b'offsets[' in msg and b'reaches beyond 4' in msg, bad
    rc, msg = _call(lib, offsets=[0, 1, 0, 0])
    assert rc == _lib.EINVAL and b'offsets[1]=(0, 0)' in msg
    for kw in ({'row0': -1}, {'rows': -1, 'hist_elems': 0, 'glcm_elems': 0, 'flags_elems': 0}):
        rc, msg = _call(lib, **kw)
        assert rc == _lib.EINVAL and b'negative row0' in msg, kw
    for kw in ({'row0': 3}, {'row0': 6, 'rows': 0, 'hist_elems': 0, 'glcm_elems': 0, 'flags_elems': 0},
               {'row0': 0x7fffffff, 'rows': 1, 'hist_elems': 16, 'glcm_elems': 512, 'flags_elems': 1}):
        rc, msg = _call(lib, **kw)
        assert rc == _lib.EINVAL and b'row0 + rows' in msg and b'R=5' in msg, kw


def test_label_texture_image_checks(lib):
    for ps in (0, 1, 2, 5, -3):
        rc, msg = _call(lib, pixel_stride=ps)
        assert rc == _lib.EINVAL and b'pixel_stride' in msg
    for rs in (0, -100):
        rc, msg = _call(lib, row_stride=rs)
        assert rc == _lib.EINVAL and b'row_stride' in msg
    for kw in ({'x0': -1}, {'y0': -1}):
        rc, msg = _call(lib, **kw)
        assert rc == _lib.EINVAL and b'negative image window origin' in msg
    # the last byte read is (y0 + 19) * 100 + (x0 + 29) * 3 + 2: one byte short, a shifted window, a wider pixel and a negative size all leave
    for kw in ({'image_bytes': 19 * 100 + 29 * 3 + 2}, {'x0': 1}, {'y0': 1}, {'pixel_stride': 4}, {'image_bytes': 0}, {'image_bytes': -5},
               {'row_stride': 1 << 62}):
        rc, msg = _call(lib, **kw)
        assert rc == _lib.EINVAL and b'image' in msg, kw
    # every check passed and rows = 0: nothing to write, no launch, whatever the other pointers
    assert _call(lib, rows=0, hist_elems=0, glcm_elems=0, flags_elems=0, map=None, extent=None, lut=None, hist=None, glcm=None, flags=None)[0] == _lib.OK


def test_zero_rows_launch_nothing(lib):
    lib.hdy_dispatch_log_reset()
    none = dict(map=None, image=None, extent=None, lut=None, hist=None, glcm=None, flags=None)
    empty = dict(rows=0, hist_elems=0, glcm_elems=0, flags_elems=0)
    assert _call(lib, **empty)[0] == _lib.OK
    assert _call(lib, **empty, **none)[0] == _lib.OK
    assert _call(lib, **empty, row0=5)[0] == _lib.OK                      # row0 + rows = R
    assert _call(lib, **empty, **none, R=0, extent_elems=0, row0=0)[0] == _lib.OK
    assert _lib.dispatch_log() == []
    assert _call(lib, **dict(empty, hist_elems=16))[0] == _lib.EINVAL     # the sizes are still checked
    assert _call(lib, **empty, levels=12)[0] == _lib.EINVAL


# ---- stain_lut --------------------------------------------------------------------------------------------------------------------------------
def _stain_coefficients(stain):
    """(3,) float64: column `stain` of the inverse of the Ruifrok-Johnston matrix (rows H, E and their cross product, each of unit length)"""
    h, e = np.array([0.65, 0.70, 0.29]), np.array([0.07, 0.99, 0.11])
    h, e = h / np.linalg.norm(h), e / np.linalg.norm(e)
    r = np.cross(h, e)
    return np.linalg.inv(np.stack([h, e, r / np.linalg.norm(r)]))[:, {'hematoxylin': 0, 'eosin': 1}[stain]]


@pytest.mark.parametrize('stain, od_max', [('hematoxylin', 2.0), ('eosin', 1.5)])
@pytest.mark.parametrize('levels', [8, 16, 32])
def test_stain_lut_gives_the_exact_level_over_all_colours(stain, od_max, levels):
    """A colour whose float64 levels * concentration / od_max lies farther than 2 * 2^-16 from an integer gets exactly clip(floor(.), 0, L - 1):
    three entries, each rounded by at most half a unit of 2^-16, account for 1.5 * 2^-16.  At most 2 000 of the 2^24 colours may lie inside
    that band and be left out (measured: 996 to 1 024 do)."""
    lut = htexture.stain_lut(stain, levels)
    assert lut.dtype == torch.int32 and tuple(lut.shape) == (3, 256) and int(lut.abs().max()) < 1 << 28
    lut = lut.numpy().astype(np.int64)
    od = -np.log10((np.arange(256) + 1) / 256.0)
    term = levels * _stain_coefficients(stain)[:, None] * od[None, :] / od_max       # (3, 256): the exact quantity is the sum of three
    band, wrong = 0, 0
    for r in range(256):
        x = term[0, r] + term[1][:, None] + term[2][None, :]
        got = np.clip((lut[0, r] + lut[1][:, None] + lut[2][None, :]) >> 16, 0, levels - 1)
        far = np.abs(x - np.rint(x)) > 2.0 / 65536
        band += far.size - int(far.sum())
        wrong += int((got != np.clip(np.floor(x), 0, levels - 1))[far].sum())
    print(f'{stain} L={levels}: {band} colours inside the band, {wrong} outside it differ')
    assert wrong == 0 and band <= 2000


def test_stain_lut_variants_and_refusals():
    for levels in (8, 16, 32):
        g = htexture.stain_lut('gray', levels).numpy().astype(np.int64)
        v = np.arange(256)
        # a grey pixel's luma is its value; v * levels / 256 is often an integer, where three roundings may fall a unit of 2^-16 short
        assert np.abs(g.sum(0) - (v * levels << 8)).max() <= 1 and (((g.sum(0) + 2) >> 16) == v * levels // 256).all()
        for c, ch in enumerate('rgb'):
            t = htexture.stain_lut(ch, levels).numpy().astype(np.int64)
            assert np.array_equal(t[c] >> 16, v * levels // 256) and not np.delete(t, c, 0).any()
    h16, r16 = htexture.stain_lut('hematoxylin', 16), htexture.stain_lut('residual', 16)
    assert not torch.equal(h16, r16) and not torch.equal(h16, htexture.stain_lut('hematoxylin', 16, od_max=1.0))
    assert torch.equal(htexture.stain_lut('eosin', 16, matrix=htexture.stain_matrix()), htexture.stain_lut('eosin', 16))
    white = h16[:, 255].sum().item()                                      # od(255) = 0: a white pixel holds no stain
    assert white == 0
    for bad in (dict(stain='dab'), dict(levels=12), dict(od_max=0.0), dict(od_max=1e-4), dict(matrix=[[1, 0, 0], [0, 1, 0], [0, 0, 1e-9]],
                                                                                              stain='residual')):
        with pytest.raises(ValueError):
            htexture.stain_lut(**bad)
