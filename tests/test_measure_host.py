"""Host side of the label measurement (csrc/measure.hip, include/hdyolo_measure.h), no GPU: the two numpy restatements of its arithmetic
(tests/measure_ref.py) against each other and against answers derived by hand, nucleus_table on CPU tensors against the numpy restatement of its
formulas, the extension header and its binding, the ABI surface of hdy_label_measure (invalid calls answered by status and message before
anything is dereferenced or launched) and the two file formats of save_nucleus_table."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import measure_ref as ref
from hd_yolo_amd import _header, _lib, build
from hd_yolo_amd import measure as hmeasure

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatements ---------------------------------------------------------------------------------------------------------------------
def test_the_two_restatements_agree_on_random_maps():
    rng = np.random.default_rng(20250115)
    for h, w, R in ((1, 1, 1), (1, 9, 3), (7, 5, 4), (13, 17, 6), (24, 31, 9)):
        for use_image, use_origin in ((False, False), (True, True), (True, False)):
            lm = ref.random_map(rng, h, w, R)
            image = rng.integers(0, 256, (h + 3, w + 5, 4), dtype=np.uint8) if use_image else None
            origin = rng.integers(-20, 20, (R, 2)).astype(np.int32) if use_origin else None
            got = ref.measure(lm, R, image, (2, 1), origin)
            want = ref.measure_slow(lm, R, image, (2, 1), origin)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (h, w, R)
            assert got[0].dtype == np.int64 and got[1].dtype == np.int32


def test_both_restatements_wrap_modulo_2_to_64():
    lm = np.zeros((3, 4), dtype=np.int32)
    origin = np.array([[-(2 ** 31), 2 ** 31 - 1]], dtype=np.int32)          # dx^2 = 2^62 and more per entry, 12 entries: the sum passes 2^64
    a, b = ref.measure(lm, 1, None, (0, 0), origin), ref.measure_slow(lm, 1, None, (0, 0), origin)
    assert np.array_equal(a[0], b[0])
    exact = sum((j + 2 ** 31) ** 2 for i in range(3) for j in range(4))
    assert exact > 2 ** 64 and int(a[0][0, 3]) == (exact + 2 ** 63) % 2 ** 64 - 2 ** 63


@pytest.mark.parametrize('a,b', [(7, 3), (3, 7), (1, 5), (4, 4)])
def test_rectangle_known_answers(a, b):
    """an axis-aligned rectangle of a columns x b rows inside a larger window: n = ab, 2 (a + b) edges, none on the border, central moments
    (a^2 - 1) / 12 and (b^2 - 1) / 12 (the variance of a, b consecutive integers), mu11 = 0"""
    lm = np.full((b + 4, a + 5), -1, dtype=np.int32)
    lm[2:2 + b, 3:3 + a] = 0
    origin = np.array([[3, 2]], dtype=np.int32)
    sums, extent = ref.measure(lm, 1, None, (0, 0), origin)
    n, sx, sy, sxx, syy, sxy, e, eb = (int(v) for v in sums[0, :8])
    assert (n, e, eb) == (a * b, 2 * (a + b), 0)
    assert extent[0].tolist() == [3, 2, 3 + a - 1, 2 + b - 1]
    assert (n * sxx - sx * sx) * 12 == (a * a - 1) * n * n and (n * syy - sy * sy) * 12 == (b * b - 1) * n * n and n * sxy - sx * sy == 0
    t = hmeasure.nucleus_table(torch.from_numpy(sums), torch.from_numpy(extent), origin=torch.from_numpy(origin), offset=(100, 200))
    np.testing.assert_allclose(float(t['major_axis'][0]), 4 * math.sqrt((max(a, b) ** 2 - 1) / 12), rtol=1e-12)
    np.testing.assert_allclose(float(t['minor_axis'][0]), 4 * math.sqrt((min(a, b) ** 2 - 1) / 12), rtol=1e-12)
    np.testing.assert_allclose(float(t['centroid_x'][0]), 100 + 3 + (a - 1) / 2, rtol=1e-12)
    np.testing.assert_allclose(float(t['centroid_y'][0]), 200 + 2 + (b - 1) / 2, rtol=1e-12)
    assert t['bbox'][0].tolist() == [103, 202, 103 + a - 1, 202 + b - 1] and not bool(t['touches_border'][0])
    if a != b:
        assert abs(float(t['orientation'][0])) == (0.0 if a > b else math.pi / 2)
    else:
        assert float(t['eccentricity'][0]) == 0.0 and float(t['compactness'][0]) == 1.0


def test_single_pixel_two_neighbours_and_the_border():
    lm = np.full((4, 6), -1, dtype=np.int32)
    lm[1, 2] = 0                      # a single pixel inside
    lm[2, 3:5], lm[3, 3:5] = 1, 2     # two 2 x 1 bars sharing a 2-edge side; label 2 lies on the bottom border
    lm[0, 0] = 3                      # the corner pixel: two of its four edges leave the window
    lm[0, 5] = 9                      # not a label (R = 5): a different neighbour, owned by nobody
    image = np.arange(4 * 6 * 3, dtype=np.uint8).reshape(4, 6, 3)
    sums, extent = ref.measure(lm, 5, image)
    assert sums[0].tolist() == [1, 2, 1, 4, 1, 2, 4, 0] + [int(v) for v in image[1, 2]] + [int(v) ** 2 for v in image[1, 2]]
    assert sums[1, [0, 6, 7]].tolist() == [2, 6, 0] and sums[2, [0, 6, 7]].tolist() == [2, 6, 2]
    assert sums[3, [0, 6, 7]].tolist() == [1, 4, 2]
    assert not sums[4].any() and extent[4].tolist() == [6, 4, -1, -1]
    assert extent[:4].tolist() == [[2, 1, 2, 1], [3, 2, 4, 2], [3, 3, 4, 3], [0, 0, 0, 0]]
    t = hmeasure.nucleus_table(torch.from_numpy(sums), torch.from_numpy(extent), offset=(10, 20))
    assert t['touches_border'].tolist() == [False, False, True, True, False]
    assert float(t['major_axis'][0]) == 0.0 and float(t['eccentricity'][0]) == 0.0 and float(t['equivalent_diameter'][0]) == math.sqrt(4 / math.pi)
    assert math.isnan(float(t['centroid_x'][4])) and math.isnan(float(t['compactness'][4])) and math.isnan(float(t['mean_rgb'][4, 0]))
    assert t['bbox'][4].tolist() == [6, 4, -1, -1] and t['bbox'][0].tolist() == [12, 21, 12, 21]


def test_nucleus_table_equals_its_numpy_restatement():
    rng = np.random.default_rng(7)
    R = 40
    lm = ref.random_map(rng, 60, 90, R, labels_above=0)
    image = rng.integers(0, 256, (70, 100, 3), dtype=np.uint8)
    origin = np.stack([rng.integers(0, 90, R), rng.integers(0, 60, R)], 1).astype(np.int32)
    sums, extent = ref.measure(lm, R, image, (4, 6), origin)
    assert (sums[:, 0] == 0).any() and (sums[:, 0] > 20).any()            # empty rows and real blobs both present
    labels, scores = torch.arange(R), torch.linspace(1, 0, R)
    t = hmeasure.nucleus_table(torch.from_numpy(sums), torch.from_numpy(extent), origin=torch.from_numpy(origin), offset=(4, 6), labels=labels,
                               scores=scores)
    ref.assert_tables_agree({k: v.numpy() for k, v in t.items()}, ref.table(sums, extent, origin, (4, 6)))
    assert t['labels'] is labels and t['scores'] is scores
    assert t['area'].dtype == torch.int64 and t['major_axis'].dtype == torch.float64 and t['touches_border'].dtype == torch.bool
    bare = hmeasure.nucleus_table(torch.from_numpy(sums), torch.from_numpy(extent), stain=False)
    assert 'mean_rgb' not in bare and 'std_rgb' not in bare and 'labels' not in bare
    with pytest.raises(ValueError, match='sums must be int64'):
        hmeasure.nucleus_table(torch.zeros((3, 13), dtype=torch.int64), torch.zeros((3, 4), dtype=torch.int32))


@pytest.mark.parametrize('ext', ['.npz', '.csv'])
def test_save_nucleus_table_round_trips(tmp_path, ext):
    rng = np.random.default_rng(3)
    R = 12
    lm = ref.random_map(rng, 30, 40, R, labels_above=0)
    image = rng.integers(0, 256, (30, 40, 3), dtype=np.uint8)
    sums, extent = ref.measure(lm, R, image)
    t = hmeasure.nucleus_table(torch.from_numpy(sums), torch.from_numpy(extent), labels=torch.arange(R) % 3, scores=torch.linspace(0.9, 0.1, R))
    path = str(tmp_path / ('nuclei' + ext))
    hmeasure.save_nucleus_table(path, t)
    back = hmeasure.load_nucleus_table(path)
    if ext == '.npz':
        assert sorted(back) == sorted(t)
        for k, v in t.items():
            assert back[k].shape == tuple(v.shape) and np.array_equal(back[k], v.numpy(), equal_nan=v.dtype.is_floating_point), k
        assert back['area'].dtype == np.int64 and back['touches_border'].dtype == bool and back['scores'].dtype == np.float32
    else:
        assert np.array_equal(back['area'], t['area'].numpy()) and back['area'].dtype == np.int64
        assert np.array_equal(back['major_axis'], t['major_axis'].numpy(), equal_nan=True)          # repr() of a float64 reads back exactly
        assert np.array_equal(back['bbox_x1'], t['bbox'][:, 2].numpy()) and np.array_equal(back['std_rgb_b'], t['std_rgb'][:, 2].numpy(), equal_nan=True)
        assert np.array_equal(back['touches_border'], t['touches_border'].numpy().astype(np.int64))
        assert np.array_equal(back['scores'], t['scores'].numpy().astype(np.float64))
    with pytest.raises(ValueError, match='neither .npz nor .csv'):
        hmeasure.save_nucleus_table(str(tmp_path / 'nuclei.txt'), t)


# ---- the extension header and the ABI surface, through the built library -------------------------------------------------------------------
FAKE = 0x10000      # an aligned non-NULL "device pointer": every call below must fail validation before anything dereferences or launches


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    from hd_yolo_amd import _ext
    return _ext.load()


def test_extension_header_parses_and_is_bound(lib):
    from hd_yolo_amd import _ext
    path = os.path.join(ROOT, 'include', 'hdyolo_measure.h')
    ext = _ext.EXTENSIONS['measure']
    assert ext.header == path
    hdr = _header.read(path)
    assert sorted(hdr.functions) == ['hdy_label_measure', 'hdy_measure_revision'] and not hdr.structs
    assert hdr.constants == {'HDY_MEASURE_REVISION': 1, 'HDY_MEASURE_COLS': 14, 'HDY_MEASURE_MAX_SIDE': 1 << 29}
    res, args = hdr.functions['hdy_label_measure']
    vp, ll, i = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int
    assert res is i and args == [vp, ll, i, i, vp, ll, ll, i, i, i, vp, vp, ll, vp, ll, i, vp]
    assert [p[0] for p in hdr.params['hdy_label_measure']][:5] == ['map', 'map_elems', 'h', 'w', 'image']
    for name, (res, args) in hdr.functions.items():
        fn = getattr(lib, name)                                            # exported by the built library ...
        assert fn.restype is res and list(fn.argtypes) == args, name      # ... and bound by _ext
        assert name not in _lib.SIGNATURES                                 # the numbered ABI does not know the extension
        assert _ext.SIGNATURES[name] == (res, args) and _ext.PARAMS[name] == hdr.params[name]
    assert (ext.functions, ext.params, ext.constants) == (hdr.functions, hdr.params, hdr.constants)
    assert (ext.revision_fn, ext.revision_macro) == ('hdy_measure_revision', 'HDY_MEASURE_REVISION')
    assert lib.hdy_measure_revision() == ext.revision == hdr.constants['HDY_MEASURE_REVISION'] == 1
    assert not any(k.startswith('HDY_MEASURE') for k in _lib.CONSTANTS)
    assert _ext.CONSTANTS['HDY_MEASURE_COLS'] == hmeasure.COLS == ref.COLS == 14


def test_every_extension_keeps_its_tables_and_a_name_belongs_to_one_header(lib):
    """the tables of every extension header side by side: what each declares, that no name is declared twice (among them or with
    include/hdyolo.h), and that the import refuses a header which breaks that"""
    from hd_yolo_amd import _ext
    want = {'measure': (['hdy_label_measure', 'hdy_measure_revision'], 3),
            'spatial': (['hdy_spatial_cells', 'hdy_spatial_density', 'hdy_spatial_neighbors', 'hdy_spatial_revision'], 6),
            'outline': (['hdy_label_hull', 'hdy_label_outline_count', 'hdy_label_outline_write', 'hdy_outline_revision'], 3),
            'graph': (['hdy_graph_knn', 'hdy_graph_mutual', 'hdy_graph_revision'], 3),
            'texture': (['hdy_label_texture', 'hdy_texture_revision'], 7)}
    assert list(_ext.EXTENSIONS) == list(want) == list(_header.EXTENSION_NAMES)                 # oldest first, texture last
    for short, (functions, n_constants) in want.items():
        ext = _ext.EXTENSIONS[short]
        assert sorted(ext.functions) == functions and sorted(ext.params) == functions and len(ext.constants) == n_constants
        assert ext.header == os.path.join(ROOT, 'include', f'hdyolo_{short}.h') == _header.extension_header(short)
        assert (ext.revision_fn, ext.revision_macro) == (f'hdy_{short}_revision', f'HDY_{short.upper()}_REVISION')
        assert ext.revision == ext.constants[ext.revision_macro] == getattr(lib, ext.revision_fn)() == 1
        assert all(k.startswith(f'HDY_{short.upper()}_') for k in ext.constants)
        for table, base in (('functions', _lib.SIGNATURES), ('constants', _lib.CONSTANTS)):
            for name in getattr(ext, table):
                assert name not in base and [s for s, e in _ext.EXTENSIONS.items() if name in getattr(e, table)] == [short], name
    exts = list(_ext.EXTENSIONS.values())
    assert _ext.SIGNATURES == {n: v for e in exts for n, v in e.functions.items()} and len(_ext.SIGNATURES) == 2 + 4 + 4 + 3 + 2
    assert _ext.PARAMS == {n: v for e in exts for n, v in e.params.items()} and sorted(_ext.PARAMS) == sorted(_ext.SIGNATURES)
    assert _ext.CONSTANTS == {n: v for e in exts for n, v in e.constants.items()} and len(_ext.CONSTANTS) == 3 + 6 + 3 + 3 + 7
    _ext.check_disjoint(_ext.EXTENSIONS)                                                         # the tables as they are pass
    graph = _ext.EXTENSIONS['graph']
    for doctored, word in ((graph._replace(functions=dict(graph.functions, hdy_spatial_cells=graph.functions['hdy_graph_mutual'])),
                            'hdy_spatial_cells is declared by include/hdyolo_spatial.h and by include/hdyolo_graph.h'),
                           (graph._replace(constants=dict(graph.constants, HDY_MEASURE_COLS=14)),
                            'HDY_MEASURE_COLS is declared by include/hdyolo_measure.h and by include/hdyolo_graph.h'),
                           (graph._replace(functions=dict(graph.functions, hdy_last_error=(ctypes.c_char_p, []))),
                            'hdy_last_error is declared by include/hdyolo.h and by include/hdyolo_graph.h'),
                           (graph._replace(constants=dict(graph.constants, HDY_ABI_VERSION=1)),
                            'HDY_ABI_VERSION is declared by include/hdyolo.h and by include/hdyolo_graph.h')):
        with pytest.raises(_lib.HdyError) as e:
            _ext.check_disjoint(dict(_ext.EXTENSIONS, graph=doctored))
        assert word in str(e.value)
    assert 'hdy_spatial_cells' not in graph.functions and 'HDY_MEASURE_COLS' not in graph.constants      # the copies were doctored, not the tables


def _call(lib, **kw):
    a = dict(map=FAKE, map_elems=20 * 30, h=20, w=30, image=None, image_bytes=0, row_stride=0, pixel_stride=0, x0=0, y0=0, origin=None, sums=FAKE,
             sums_elems=14 * 5, extent=FAKE, extent_elems=4 * 5, R=5)
    a.update(kw)
    rc = lib.hdy_label_measure(a['map'], a['map_elems'], a['h'], a['w'], a['image'], a['image_bytes'], a['row_stride'], a['pixel_stride'], a['x0'],
                               a['y0'], a['origin'], a['sums'], a['sums_elems'], a['extent'], a['extent_elems'], a['R'], None)
    return rc, lib.hdy_last_error()


def test_label_measure_argument_checks(lib):
    for kw in ({'map': None}, {'sums': None}, {'extent': None}):
        rc, msg = _call(lib, **kw)
        assert rc == _lib.EINVAL and b'null' in msg, kw
    for kw in ({'sums': FAKE + 4}, {'map': FAKE + 2}, {'origin': FAKE + 1}, {'extent': FAKE + 2}):
        rc, msg = _call(lib, **kw)
        assert rc == _lib.EINVAL and b'misaligned' in msg, kw
    for kw in ({'R': -1, 'sums_elems': -14, 'extent_elems': -4}, {'map_elems': -600}, {'sums_elems': -1}, {'extent_elems': -1}):
        rc, msg = _call(lib, **kw)
        assert rc == _lib.EINVAL and b'negative' in msg, kw
    for kw in ({'h': 0, 'map_elems': 0}, {'w': -5}, {'h': (1 << 29) + 1, 'w': 1, 'map_elems': (1 << 29) + 1}):
        rc, msg = _call(lib, **kw)
        assert rc == _lib.EINVAL and b'outside [1, 536870912]' in msg, kw
    for n in (599, 601, 0):
        rc, msg = _call(lib, map_elems=n)
        assert rc == _lib.EINVAL and b'map_elems' in msg
    # 64-bit sizes: a 70 000 x 70 000 window is 4.9e9 entries; the count that 32-bit arithmetic would give is refused, the true one is not
    rc, msg = _call(lib, h=70000, w=70000, map_elems=(70000 * 70000) & 0xFFFFFFFF)
    assert rc == _lib.EINVAL and b'map_elems' in msg
    rc, msg = _call(lib, h=70000, w=70000, map_elems=70000 * 70000, sums_elems=1)
    assert rc == _lib.EINVAL and b'sums_elems' in msg
    for n in (69, 71, 0):
        rc, msg = _call(lib, sums_elems=n)
        assert rc == _lib.EINVAL and b'sums_elems' in msg
    for n in (19, 21, 0):
        rc, msg = _call(lib, extent_elems=n)
        assert rc == _lib.EINVAL and b'extent_elems' in msg


def test_label_measure_image_checks(lib):
    ok = dict(image=FAKE + 1, image_bytes=19 * 100 + 29 * 3 + 3, row_stride=100, pixel_stride=3)     # a byte pointer needs no alignment
    for ps in (0, 1, 2, 5, -3):
        rc, msg = _call(lib, **dict(ok, pixel_stride=ps))
        assert rc == _lib.EINVAL and b'pixel_stride' in msg
    for rs in (0, -100):
        rc, msg = _call(lib, **dict(ok, row_stride=rs))
        assert rc == _lib.EINVAL and b'row_stride' in msg
    for kw in ({'x0': -1}, {'y0': -1}):
        rc, msg = _call(lib, **dict(ok, **kw))
        assert rc == _lib.EINVAL and b'negative image window origin' in msg
    # the last byte read is (y0 + 19) * 100 + (x0 + 29) * 3 + 2: one byte short, a shifted window, a wider pixel and a negative size all leave
    for kw in ({'image_bytes': ok['image_bytes'] - 1}, {'x0': 1}, {'y0': 1}, {'pixel_stride': 4}, {'image_bytes': 0}, {'image_bytes': -5},
               {'row_stride': 1 << 62}):
        rc, msg = _call(lib, **dict(ok, **kw))
        assert rc == _lib.EINVAL and b'image' in msg, kw
    # every check passed and R = 0: nothing to write, no launch, whatever the output pointers
    assert _call(lib, **dict(ok, R=0, sums=None, extent=None, map=None, sums_elems=0, extent_elems=0))[0] == _lib.OK


def test_zero_rows_launch_nothing(lib):
    lib.hdy_dispatch_log_reset()
    assert _call(lib, R=0, sums_elems=0, extent_elems=0)[0] == _lib.OK
    assert _call(lib, R=0, sums_elems=0, extent_elems=0, sums=None, extent=None, map=None)[0] == _lib.OK
    assert _lib.dispatch_log() == []
    assert _call(lib, R=0, sums_elems=14, extent_elems=0)[0] == _lib.EINVAL          # the sizes are still checked
