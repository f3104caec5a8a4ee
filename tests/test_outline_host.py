"""Host side of the outlines and hulls (csrc/outline.hip, include/hdyolo_outline.h), no GPU: the restatement (tests/outline_ref.py) against
answers derived by hand, against its own slow second form (the polygon rasterised by the even-odd rule) and against measure_ref on random
maps, its hull against scipy.spatial.ConvexHull, shape_table on CPU tensors against a per-row restatement, the two file formats of
save_polygons, the extension header and its binding, and the ABI surface of the three entry points (invalid calls answered by status and
message before anything is dereferenced or launched)."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch
from scipy.spatial import ConvexHull

import measure_ref as mref
import outline_ref as ref
from test_measure_host import _call as _measure      # the same 20 x 30 map of 5 labels as COMMON below
from test_texture_host import _call as _texture
from hd_yolo_amd import _header, _lib, build
from hd_yolo_amd import outline as houtline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(ref.HAND))
def test_hand_answers(name):
    """a single pixel, a 1 x 5 row, L, U and plus shapes, a 3 x 3 ring (outline of the outer square, enclosed 9, n 8, not simple), two diagonal
    pixels of one label (the first pixel only, not simple), a ring whose hole leaks out through a diagonal gap, a label on every window border"""
    lm, verts, area2, L, n, simple, hi, hf = ref.HAND[name]
    for pad in (0, 3):                                                     # on every window border, and inside a larger window
        m = np.pad(lm, pad, constant_values=-1)
        sums, extent = mref.measure(m, 1)
        v, a2, cracks, flag = ref.outline(m, 0, extent[0])
        assert (v - pad).tolist() == [list(p) for p in verts] and (a2, cracks, flag) == (area2, L, 0) and v.dtype == np.int32
        assert int(sums[0, 0]) == n and (a2 // 2 == n and cracks == int(sums[0, 6])) == simple
        got_i, got_f = ref.hull(m, 0, extent[0])
        assert got_i == tuple(hi) + (0,)
        np.testing.assert_allclose(got_f, hf, rtol=1e-12)
        K, F, (top, left) = ref.filled_component(m, 0, int(extent[0, 1]), int(v[0, 0]))
        assert int(F.sum()) == a2 // 2 and np.array_equal(ref.rasterise(v - [left, top], *F.shape), F)
    assert len(verts) % 2 == 0 and len(verts) >= 4


def test_flags_of_the_restatement():
    lm = np.full((6, 1100), -1, dtype=np.int32)
    lm[2, 10:10 + 1025] = 0
    lm[4, 5:8] = 1
    lm[3:6, 20:23] = 2
    lm[4, 21] = -1                                                         # label 2: a ring
    extent = mref.measure(lm, 4)[1]
    assert ref.outline(lm, 0, extent[0])[1:] == (0, 0, 2) and ref.hull(lm, 0, extent[0]) == ((0, 0, 0, 2), (0.0, 0.0))
    assert ref.outline(lm, 3, extent[3])[1:] == (0, 0, 1) and ref.hull(lm, 3, extent[3])[0] == (0, 0, 0, 1)
    assert ref.outline(lm, 1, extent[1])[1:] == (6, 8, 0)
    assert ref.outline(lm, 1, extent[2])[1:] == (0, 0, 4) and ref.hull(lm, 1, extent[2])[0] == (0, 0, 0, 4)      # another label's box: no entry
    assert ref.outline(lm, 1, [6, 4, 7, 4])[1:] == (0, 0, 4)              # the entry to the left of s is the label's
    assert ref.outline(lm, 1, [5, 4, 5, 4])[1:] == (0, 0, 4)              # a box of one pixel: the walk takes 8 cracks, the box has 4 edges
    assert ref.outline(lm, 2, [21, 5, 22, 5])[1:] == (0, 0, 4)            # s = (5, 21) below the hole: its top edge is no edge of the filled ring
    assert ref.outline(lm, 2, extent[2])[1:] == (18, 12, 0)
    assert ref.clamped_box([-5, -5, 2000, 3], 6, 1100) == (0, 0, 1100, 4, 2) and ref.clamped_box([7, 2, 6, 2], 6, 1100)[4] == 1


def test_random_maps_shoelace_raster_and_edges():
    rng = np.random.default_rng(20250301)
    seen_simple = seen_other = 0
    for h, w, R in ((1, 1, 1), (1, 9, 3), (7, 5, 4), (13, 17, 6), (24, 31, 9), (40, 60, 12)):
        lm = mref.random_map(rng, h, w, R)
        sums, extent = mref.measure(lm, R)
        for r in range(R):
            v, area2, L, flag = ref.outline(lm, r, extent[r])
            if sums[r, 0] == 0:
                assert flag == 1 and len(v) == 0
                continue
            assert flag == 0 and len(v) >= 4 and len(v) % 2 == 0 and v[0].tolist() == [int(np.nonzero(lm[extent[r, 1]] == r)[0][0]), int(extent[r, 1])]
            K, F, (top, left) = ref.filled_component(lm, r, int(v[0, 1]), int(v[0, 0]))
            assert area2 == 2 * int(F.sum())                                                          # shoelace == 2 |filled|
            assert np.array_equal(ref.rasterise(v - [left, top], *F.shape), F)                       # rasterised polygon == filled component
            steps = np.abs(np.roll(v, -1, 0) - v)
            assert (steps.min(1) == 0).all() and int(steps.sum()) == L                               # axis-parallel edges; L is their length
            if area2 // 2 == sums[r, 0] and int(K.sum()) == sums[r, 0]:                              # one component, no hole: simple
                assert L == sums[r, 6]
                seen_simple += 1
            else:
                seen_other += 1
    assert seen_simple > 5 and seen_other > 5


def test_hull_against_qhull():
    rng = np.random.default_rng(5)
    R = 9
    lm = mref.random_map(rng, 40, 60, R)
    sums, extent = mref.measure(lm, R)
    checked = 0
    for r in range(R):
        if sums[r, 0] == 0:
            continue
        (H, area2, fmax2, flag), (perimeter, fmin) = ref.hull(lm, r, extent[r])
        ii, jj = np.nonzero(lm == r)
        corners = np.unique(np.concatenate([np.stack([jj + a, ii + b], 1) for a in (0, 1) for b in (0, 1)]), axis=0).astype(np.float64)
        q = ConvexHull(corners)                                            # 2-D: .volume is the area, .area the perimeter
        np.testing.assert_allclose(area2 / 2, q.volume, rtol=1e-9)
        np.testing.assert_allclose(perimeter, q.area, rtol=1e-9)
        # Qhull's default options merge coplanar facets, so its vertices are the strict corners too; where it keeps a collinear point the
        # area and the perimeter above have still been compared
        if len(q.vertices) == H:
            checked += 1
        d = corners[:, None, :] - corners[None, :, :]
        assert fmax2 == int((d * d).sum(2).max()) and flag == 0
        # the smallest width over all directions is attained on an edge's normal: no direction of a fine fan does better
        ang = np.linspace(0, math.pi, 721)
        proj = corners @ np.stack([np.cos(ang), np.sin(ang)])
        assert fmin <= (proj.max(0) - proj.min(0)).min() + 1e-9
    assert checked >= 3


# ---- shape_table and the files ---------------------------------------------------------------------------------------------------------------
def _case(seed=7, R=30):
    rng = np.random.default_rng(seed)
    lm = mref.random_map(rng, 50, 80, R, labels_above=0)
    lm[0, 0] = -1
    sums, extent = mref.measure(lm, R)
    extent[3], extent[5] = (80, 50, -1, -1), (0, 0, 0, 0)                  # two flagged rows: an empty box (1), a box without the label (4)
    return lm, sums, extent, ref.outlines(lm, R, extent), ref.hulls(lm, R, extent)


def test_shape_table_equals_its_per_row_restatement():
    lm, sums, extent, (offsets, verts, counts), (hull_i, hull_f) = _case()
    assert (sums[:, 0] == 0).any() and counts[3, 3] == 1 and counts[5, 3] == 4 and (counts[:, 3] == 0).sum() > 10
    t = houtline.shape_table(*(torch.from_numpy(a) for a in (sums, counts, hull_i, hull_f)))
    assert tuple(t) == houtline.SHAPE_COLUMNS
    assert t['simple'].dtype == torch.bool and t['enclosed_area'].dtype == torch.int64 and t['solidity'].dtype == torch.float64
    for r in range(len(sums)):
        row = ref.shape_row(int(sums[r, 0]), int(sums[r, 6]), counts[r], hull_i[r], hull_f[r])
        for k, v in row.items():
            got = t[k][r].item()
            assert (math.isnan(got) and math.isnan(v)) if isinstance(v, float) and math.isnan(v) else got == pytest.approx(v, rel=1e-12), (r, k)
    ok = (sums[:, 0] > 0) & (counts[:, 3] == 0)
    assert bool(torch.isnan(t['solidity'][torch.from_numpy(~ok)]).all()) and not bool(t['simple'][torch.from_numpy(~ok)].any())
    sol = t['solidity'][torch.from_numpy(ok)]
    assert bool(((sol > 0) & (sol <= 1)).all()) and bool((t['feret_ratio'][torch.from_numpy(ok)] <= 1).all())
    with pytest.raises(ValueError, match='counts must be'):
        houtline.shape_table(torch.from_numpy(sums), torch.from_numpy(counts[:, :3]), torch.from_numpy(hull_i), torch.from_numpy(hull_f))


@pytest.mark.parametrize('ext', ['.npz', '.geojson'])
def test_save_polygons_round_trips(tmp_path, ext):
    lm, sums, extent, (offsets, verts, counts), _ = _case(seed=3, R=12)
    R = len(sums)
    labels, scores = torch.arange(R) % 3, torch.linspace(0.9, 0.1, R)
    path = str(tmp_path / ('nuclei' + ext))
    houtline.save_polygons(path, torch.from_numpy(offsets), torch.from_numpy(verts), offset=(100, 200), scale=0.5, labels=labels, scores=scores)
    back = houtline.load_polygons(path)
    if ext == '.npz':
        assert np.array_equal(back['offsets'], offsets) and np.array_equal(back['verts'], verts) and back['verts'].dtype == np.int32
        assert back['offset'].tolist() == [100.0, 200.0] and float(back['scale']) == 0.5 and np.array_equal(back['labels'], labels.numpy())
    else:
        with open(path) as f:
            doc = json.load(f)
        rows = np.nonzero(counts[:, 0])[0]
        assert doc['type'] == 'FeatureCollection' and len(doc['features']) == len(rows) < R
        first = doc['features'][0]
        ring = first['geometry']['coordinates'][0]
        assert first['type'] == 'Feature' and first['geometry']['type'] == 'Polygon' and ring[0] == ring[-1] and len(ring) == counts[rows[0], 0] + 1
        assert first['properties'] == {'row': int(rows[0]), 'classification': int(labels[rows[0]]), 'score': float(scores[rows[0]].double())}
        assert np.array_equal(back['rows'], rows) and np.array_equal(back['offsets'], np.concatenate([[0], np.cumsum(counts[rows, 0])]))
        assert np.array_equal(back['verts'], (verts.astype(np.float64) + [100.0, 200.0]) / 0.5)
        assert np.array_equal(back['labels'], labels.numpy()[rows]) and np.array_equal(back['scores'], scores.double().numpy()[rows])
    with pytest.raises(ValueError, match='neither .npz nor .geojson'):
        houtline.save_polygons(str(tmp_path / 'nuclei.txt'), offsets, verts)
    with pytest.raises(ValueError, match='offsets do not describe'):
        houtline.save_polygons(path, offsets[:-1], verts)


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
    path = os.path.join(ROOT, 'include', 'hdyolo_outline.h')
    ext = _ext.EXTENSIONS['outline']
    assert ext.header == path
    hdr = _header.read(path)
    assert sorted(hdr.functions) == ['hdy_label_hull', 'hdy_label_outline_count', 'hdy_label_outline_write', 'hdy_outline_revision']
    assert not hdr.structs
    assert hdr.constants == {'HDY_OUTLINE_REVISION': 1, 'HDY_OUTLINE_MAX_SIDE': 1024, 'HDY_OUTLINE_MAX_WINDOW': 1 << 29}
    vp, ll, i = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int
    assert hdr.functions['hdy_outline_revision'] == (i, [])
    assert hdr.functions['hdy_label_outline_count'] == (i, [vp, ll, i, i, vp, ll, i, vp, ll, vp])
    assert hdr.functions['hdy_label_outline_write'] == (i, [vp, ll, i, i, vp, ll, i, vp, ll, vp, ll, vp, vp])
    assert hdr.functions['hdy_label_hull'] == (i, [vp, ll, i, i, vp, ll, i, vp, ll, vp, ll, vp])
    assert [p[0] for p in hdr.params['hdy_label_outline_write']] == ['map', 'map_elems', 'h', 'w', 'extent', 'extent_elems', 'R', 'offsets',
                                                                     'offsets_elems', 'verts', 'verts_elems', 'status', 'stream']
    for name, (res, args) in hdr.functions.items():
        fn = getattr(lib, name)                                            # exported by the built library ...
        assert fn.restype is res and list(fn.argtypes) == args, name      # ... and bound by _ext
        assert name not in _lib.SIGNATURES                                 # the numbered ABI does not know the extension
        assert _ext.SIGNATURES[name] == (res, args) and _ext.PARAMS[name] == hdr.params[name]
    assert (ext.functions, ext.params, ext.constants) == (hdr.functions, hdr.params, hdr.constants)
    assert (ext.revision_fn, ext.revision_macro) == ('hdy_outline_revision', 'HDY_OUTLINE_REVISION')
    assert lib.hdy_outline_revision() == ext.revision == 1 and _ext.CONSTANTS['HDY_OUTLINE_MAX_SIDE'] == ref.MAX_SIDE == 1024
    assert not any(k.startswith('HDY_OUTLINE') for k in _lib.CONSTANTS)


COMMON = dict(map=FAKE, map_elems=20 * 30, h=20, w=30, extent=FAKE, extent_elems=4 * 5, R=5)


def _count(lib, **kw):
    a = dict(COMMON, counts=FAKE, counts_elems=4 * 5)
    a.update(kw)
    rc = lib.hdy_label_outline_count(a['map'], a['map_elems'], a['h'], a['w'], a['extent'], a['extent_elems'], a['R'], a['counts'], a['counts_elems'],
                                     None)
    return rc, lib.hdy_last_error()


def _write(lib, **kw):
    a = dict(COMMON, offsets=FAKE, offsets_elems=6, verts=FAKE, verts_elems=2 * 40, status=FAKE)
    a.update(kw)
    rc = lib.hdy_label_outline_write(a['map'], a['map_elems'], a['h'], a['w'], a['extent'], a['extent_elems'], a['R'], a['offsets'],
                                     a['offsets_elems'], a['verts'], a['verts_elems'], a['status'], None)
    return rc, lib.hdy_last_error()


def _hull(lib, **kw):
    a = dict(COMMON, hull_i=FAKE, hull_i_elems=4 * 5, hull_f=FAKE, hull_f_elems=2 * 5)
    a.update(kw)
    rc = lib.hdy_label_hull(a['map'], a['map_elems'], a['h'], a['w'], a['extent'], a['extent_elems'], a['R'], a['hull_i'], a['hull_i_elems'],
                            a['hull_f'], a['hull_f_elems'], None)
    return rc, lib.hdy_last_error()


@pytest.mark.parametrize('call', [_count, _write, _hull, _measure, _texture], ids=['count', 'write', 'hull', 'measure', 'texture'])
def test_the_checks_all_three_share(lib, call):
    """the map and extent checks of csrc/label_common.h, through the three entry points here and those of hdy_label_measure and hdy_label_texture"""
    lib.hdy_dispatch_log_reset()
    for kw in ({'map': None}, {'extent': None}):
        rc, msg = call(lib, **kw)
        assert rc == _lib.EINVAL and b'null' in msg, kw
    for kw in ({'map': FAKE + 2}, {'extent': FAKE + 1}):
        rc, msg = call(lib, **kw)
        assert rc == _lib.EINVAL and b'misaligned' in msg, kw
    for kw in ({'R': -1}, {'map_elems': -600}, {'extent_elems': -1}):
        rc, msg = call(lib, **kw)
        assert rc == _lib.EINVAL and b'negative' in msg, kw
    for kw in ({'h': 0, 'map_elems': 0}, {'w': -5}, {'h': (1 << 29) + 1, 'w': 1, 'map_elems': (1 << 29) + 1}):
        rc, msg = call(lib, **kw)
        assert rc == _lib.EINVAL and b'outside [1, 536870912]' in msg, kw
    for n in (599, 601, 0, (70000 * 70000) & 0xFFFFFFFF):
        rc, msg = call(lib, map_elems=n, **({'h': 70000, 'w': 70000} if n > 601 else {}))
        assert rc == _lib.EINVAL and b'map_elems' in msg
    for n in (19, 21, 0):
        rc, msg = call(lib, extent_elems=n)
        assert rc == _lib.EINVAL and b'extent_elems' in msg
    assert _lib.dispatch_log() == []


def test_outline_count_argument_checks(lib):
    lib.hdy_dispatch_log_reset()
    for kw, word in (({'counts': None}, b'null'), ({'counts': FAKE + 4}, b'misaligned'), ({'counts_elems': -1}, b'negative'),
                     ({'counts_elems': 19}, b'counts_elems'), ({'counts_elems': 21}, b'counts_elems'), ({'counts_elems': 0}, b'counts_elems')):
        rc, msg = _count(lib, **kw)
        assert rc == _lib.EINVAL and word in msg, kw
    assert _count(lib, R=0, extent_elems=0, counts_elems=0, map=None, extent=None, counts=None)[0] == _lib.OK
    assert _count(lib, R=0, extent_elems=0, counts_elems=4)[0] == _lib.EINVAL                         # the sizes are still checked
    assert _lib.dispatch_log() == []


def test_outline_write_argument_checks(lib):
    lib.hdy_dispatch_log_reset()
    for kw, word in (({'offsets': None}, b'null'), ({'status': None}, b'null'), ({'verts': None}, b'null'), ({'offsets': FAKE + 4}, b'misaligned'),
                     ({'verts': FAKE + 2}, b'misaligned'), ({'status': FAKE + 1}, b'misaligned'), ({'offsets_elems': -1}, b'negative'),
                     ({'verts_elems': -2}, b'negative'), ({'offsets_elems': 5}, b'offsets_elems'), ({'offsets_elems': 7}, b'offsets_elems'),
                     ({'verts_elems': 81}, b'odd')):
        rc, msg = _write(lib, **kw)
        assert rc == _lib.EINVAL and word in msg, kw
    assert _write(lib, R=0, extent_elems=0, offsets_elems=1, verts_elems=0, map=None, extent=None, offsets=None, verts=None, status=None)[0] == _lib.OK
    assert _write(lib, R=0, extent_elems=0, offsets_elems=0)[0] == _lib.EINVAL
    assert _lib.dispatch_log() == []


def test_hull_argument_checks(lib):
    lib.hdy_dispatch_log_reset()
    for kw, word in (({'hull_i': None}, b'null'), ({'hull_f': None}, b'null'), ({'hull_i': FAKE + 4}, b'misaligned'), ({'hull_f': FAKE + 4}, b'misaligned'),
                     ({'hull_i_elems': -1}, b'negative'), ({'hull_f_elems': -1}, b'negative'), ({'hull_i_elems': 19}, b'hull_i_elems'),
                     ({'hull_f_elems': 11}, b'hull_f_elems'), ({'hull_f_elems': 20}, b'hull_f_elems')):
        rc, msg = _hull(lib, **kw)
        assert rc == _lib.EINVAL and word in msg, kw
    assert _hull(lib, R=0, extent_elems=0, hull_i_elems=0, hull_f_elems=0, map=None, extent=None, hull_i=None, hull_f=None)[0] == _lib.OK
    assert _hull(lib, R=0, extent_elems=0, hull_i_elems=0, hull_f_elems=2)[0] == _lib.EINVAL
    assert _lib.dispatch_log() == []
