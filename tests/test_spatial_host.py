"""Host side of the neighbourhood features (csrc/spatial.hip, include/hdyolo_spatial.h), no GPU: the numpy restatement (tests/spatial_ref.py)
against a plain double loop and against answers derived by hand, to_units / interaction_matrix / neighborhood on CPU tensors where they need no
kernel, the extension header and its binding, and the ABI surface of the three entry points (invalid calls answered by status and message
before anything is dereferenced or launched)."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import spatial_ref as ref
from hd_yolo_amd import _header, _lib, build
from hd_yolo_amd import spatial

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a, b))


def test_restatement_equals_a_double_loop():
    rng = np.random.default_rng(20250301)
    for N, C, radii in ((1, 1, (5,)), (2, 2, (3, 9)), (37, 3, (20, 45, 90)), (60, 16, (10, 30, 60, 120)), (60, 3, (40, 41))):
        xy = rng.integers(0, 300, (N, 2)).astype(np.int32)
        cls = rng.integers(-1, C + 1, N).astype(np.int32)
        xy[rng.integers(0, N, N // 6)] = -1                                   # some absent
        if N > 10:
            xy[5:9] = xy[4]                                                  # coincident points
        assert _same(ref.neighbors(xy, cls, C, radii, chunk=7), ref.neighbors_slow(xy, cls, C, radii)), (N, C)
    xy, cls = ref.mixed(rng, 60, 8, 3)
    got = ref.neighbors(xy, cls, 3, (32, 64))
    assert _same(got, ref.neighbors_slow(xy, cls, 3, (32, 64)))
    assert got[0].dtype == np.int32 and got[1].dtype == np.int64 and got[2].dtype == np.int32


def test_exactly_r_counts_and_one_unit_more_does_not():
    r = 480
    for d, want in ((r, 1), (r + 1, 0)):
        xy = np.array([[100, 100], [100 + d, 100]], dtype=np.int32)
        counts, d2, row = ref.neighbors(xy, [0, 0], 1, (r,))
        assert counts[:, 0, 0].tolist() == [want, want]
        assert d2[:, 0].tolist() == ([r * r, r * r] if want else [-1, -1]) and row[:, 0].tolist() == ([1, 0] if want else [-1, -1])
    # a 3-4-5 triangle scaled: d2 = 300^2 + 400^2 = 500^2 exactly
    counts, d2, _ = ref.neighbors(np.array([[0, 0], [300, 400]]), [0, 1], 2, (499, 500))
    assert counts[0].tolist() == [[0, 0], [0, 1]] and counts[1].tolist() == [[0, 0], [1, 0]] and d2.tolist() == [[-1, 250000], [250000, -1]]


def test_three_coincident_points():
    xy = np.full((3, 2), 77, dtype=np.int32)
    counts, d2, row = ref.neighbors(xy, [0, 0, 1], 2, (1, 2))
    # a point is not its own neighbour, by identity: the others at the same place count, with d2 = 0
    assert counts[:, 0].tolist() == [[1, 1], [1, 1], [2, 0]] and np.array_equal(counts[:, 0], counts[:, 1])
    assert d2.tolist() == [[0, 0], [0, 0], [0, -1]] and row.tolist() == [[1, 2], [0, 2], [0, -1]]


def test_tie_rule_lowest_row_wins():
    # rows 1..4 all at distance 10 from row 0; row 5 of the same class is nearer to nobody but row 0's tie is decided by the row number
    xy = np.array([[50, 50], [60, 50], [40, 50], [50, 60], [50, 40]], dtype=np.int32)
    _, d2, row = ref.neighbors(xy, [0, 1, 1, 1, 1], 2, (10,))
    assert d2[0].tolist() == [-1, 100] and row[0].tolist() == [-1, 1]
    perm = [0, 4, 3, 2, 1]
    _, d2p, rowp = ref.neighbors(xy[perm], [0, 1, 1, 1, 1], 2, (10,))
    assert d2p[0].tolist() == [-1, 100] and rowp[0].tolist() == [-1, 1]        # still the lowest ROW, which is now another point
    assert _same(ref.neighbors_slow(xy, [0, 1, 1, 1, 1], 2, (10,)), ref.neighbors(xy, [0, 1, 1, 1, 1], 2, (10,)))


def test_query_only_and_absent_points():
    xy = np.array([[10, 10], [12, 10], [14, 10], [-1, 10], [10, -5]], dtype=np.int32)
    cls = np.array([0, -1, 2 ** 31 - 1, 0, 0], dtype=np.int64)
    counts, d2, row = ref.neighbors(xy, cls, 1, (8,))
    assert counts[:, 0, 0].tolist() == [0, 1, 1, 0, 0]                        # rows 1 and 2 see row 0; nobody sees them; rows 3, 4 are absent
    assert d2[:, 0].tolist() == [-1, 4, 16, -1, -1] and row[:, 0].tolist() == [-1, 0, 0, -1, -1]
    grid = ref.density(xy, cls, 1, 8, 2, 2)
    assert grid[:, :, 0].tolist() == [[0, 0], [0, 1]]                         # only row 0 is counted: x = y = 10 -> field (1, 1)


# ---- to_units, interaction_matrix, neighborhood on CPU tensors --------------------------------------------------------------------------------
def test_to_units_halves_negatives_and_nan():
    px = torch.tensor([[0.0, 1.0], [0.03125, 0.09375], [2.5, -0.5], [-0.03, 1e6], [float('nan'), 3.0], [float('inf'), -float('inf')], [1e12, 7.0]])
    u = spatial.to_units(px)
    assert u.dtype == torch.int32
    # 0.03125 * 16 = 0.5 and 0.09375 * 16 = 1.5: ties go to even (torch.round); -0.03 * 16 = -0.48 rounds to 0 and stays present
    assert u.tolist() == [[0, 16], [0, 2], [40, -8], [0, 16000000], [-1, 48], [-1, -1], [-1, 112]]
    assert spatial.to_units(torch.tensor([3, 5])).tolist() == [48, 80] and spatial.to_units(torch.tensor([1.25], dtype=torch.float64)).tolist() == [20]
    assert spatial.radius_units(30) == 480 and spatial.radius_units(0.03125) == 0 and spatial.UNITS == ref.UNITS


def test_interaction_matrix_on_cpu():
    rng = np.random.default_rng(5)
    N, K, C = 200, 3, 4
    counts = rng.integers(0, 50, (N, K, C)).astype(np.int32)
    cls = rng.integers(-1, C + 1, N)
    got = spatial.interaction_matrix(torch.from_numpy(counts), torch.from_numpy(cls), C)
    assert got.dtype == torch.int64 and tuple(got.shape) == (K, C, C) and np.array_equal(got.numpy(), ref.interaction(counts, cls, C))
    # on true counts the matrix of one symmetric relation is symmetric: pairs (a, b) = pairs (b, a)
    xy, cl = ref.uniform(rng, 300, 64, 3)
    c3 = ref.neighbors(xy, cl, 3, (100, 300))[0]
    m = spatial.interaction_matrix(torch.from_numpy(c3), torch.from_numpy(cl), 3).numpy()
    assert np.array_equal(m, m.transpose(0, 2, 1)) and m[1].sum() > m[0].sum() > 0
    assert tuple(spatial.interaction_matrix(torch.zeros((0, 2, 3), dtype=torch.int32), torch.zeros((0,), dtype=torch.int64), 3).shape) == (2, 3, 3)
    with pytest.raises(ValueError, match='do not describe'):
        spatial.interaction_matrix(torch.zeros((4, 2, 3), dtype=torch.int32), torch.zeros((5,), dtype=torch.int64), 3)


def test_neighborhood_column_shapes_without_rows():
    empty = {'centroid_x': torch.zeros(0, dtype=torch.float64), 'centroid_y': torch.zeros(0, dtype=torch.float64), 'area': torch.zeros(0, dtype=torch.int64),
             'labels': torch.zeros(0, dtype=torch.int64)}
    out = spatial.neighborhood(empty, 5, (32, 64), field_px=256, size=(1000, 520))
    assert sorted(out) == ['density', 'nearest_dist', 'nearest_row', 'neighbors']
    assert tuple(out['neighbors'].shape) == (0, 2, 5) and out['neighbors'].dtype == torch.int32
    assert tuple(out['nearest_dist'].shape) == (0, 5) and out['nearest_dist'].dtype == torch.float64
    assert tuple(out['nearest_row'].shape) == (0, 5) and out['nearest_row'].dtype == torch.int32
    assert tuple(out['density'].shape) == (4, 3, 5) and out['density'].dtype == torch.int32 and not bool(out['density'].any())
    boxes_only = {'boxes': torch.zeros((0, 4)), 'labels': torch.zeros(0, dtype=torch.int64)}
    assert sorted(spatial.neighborhood(boxes_only, 2, (8,))) == ['nearest_dist', 'nearest_row', 'neighbors']
    with pytest.raises(ValueError, match="no 'labels'"):
        spatial.neighborhood({'boxes': torch.zeros((0, 4))}, 2, (8,))
    with pytest.raises(ValueError, match='neither a nucleus table'):
        spatial.neighborhood({'labels': torch.zeros(0, dtype=torch.int64)}, 2, (8,))
    # the points of a table: centroids in units, rows of area 0 absent, labels - 1 with everything outside 0 .. nc - 1 as -1
    t = {'centroid_x': torch.tensor([1.5, 2.0, float('nan'), 4.0]), 'centroid_y': torch.tensor([0.25, 2.0, 1.0, 4.0]), 'area': torch.tensor([3, 0, 0, 9]),
         'labels': torch.tensor([1, 2, 1, 4])}
    xy, cls = spatial._points(t, 3)
    assert xy.tolist() == [[24, 4], [-1, -1], [-1, -1], [64, 64]] and cls.tolist() == [0, 1, 0, -1]
    xy, cls = spatial._points({'boxes': torch.tensor([[0.0, 2.0, 3.0, 4.0]]), 'labels': torch.tensor([0])}, 3)
    assert xy.tolist() == [[24, 48]] and cls.tolist() == [-1]


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
    path = os.path.join(ROOT, 'include', 'hdyolo_spatial.h')
    ext = _ext.EXTENSIONS['spatial']
    assert ext.header == path
    hdr = _header.read(path)
    assert sorted(hdr.functions) == ['hdy_spatial_cells', 'hdy_spatial_density', 'hdy_spatial_neighbors', 'hdy_spatial_revision'] and not hdr.structs
    assert hdr.constants == {'HDY_SPATIAL_REVISION': 1, 'HDY_SPATIAL_SUBPIXEL': 16, 'HDY_SPATIAL_MAX_CLASSES': 16, 'HDY_SPATIAL_MAX_RADII': 4,
                             'HDY_SPATIAL_MAX_COORD': 1 << 26, 'HDY_SPATIAL_MAX_CELLS': 1 << 24}
    vp, ll, i = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int
    assert hdr.functions['hdy_spatial_cells'] == (i, [vp, ll, i, i, i, i, vp, ll, vp, ll, vp])
    assert hdr.functions['hdy_spatial_neighbors'] == (i, [vp, ll, i, vp, ll, i, i, i, vp, i, i, vp, ll, vp, ll, vp, ll, vp])
    assert hdr.functions['hdy_spatial_density'] == (i, [vp, ll, i, i, i, i, i, vp, ll, vp])
    assert [p[0] for p in hdr.params['hdy_spatial_neighbors']][:5] == ['pts', 'pts_elems', 'N', 'cell_start', 'cell_start_elems']
    for name, (res, args) in hdr.functions.items():
        fn = getattr(lib, name)                                            # exported by the built library ...
        assert fn.restype is res and list(fn.argtypes) == args, name      # ... and bound by _ext
        assert name not in _lib.SIGNATURES                                 # the numbered ABI does not know the extension
        assert _ext.SIGNATURES[name] == (res, args) and _ext.PARAMS[name] == hdr.params[name]
    assert (ext.functions, ext.params, ext.constants) == (hdr.functions, hdr.params, hdr.constants)
    assert (ext.revision_fn, ext.revision_macro) == ('hdy_spatial_revision', 'HDY_SPATIAL_REVISION')
    assert lib.hdy_spatial_revision() == ext.revision == 1
    c = _ext.CONSTANTS
    assert c['HDY_SPATIAL_SUBPIXEL'] == spatial.UNITS and (c['HDY_SPATIAL_MAX_CLASSES'], c['HDY_SPATIAL_MAX_RADII']) == (16, 4)
    assert not any(k.startswith('HDY_SPATIAL') for k in _lib.CONSTANTS)


def _radii(*r):
    return (ctypes.c_int * len(r))(*r)


def _cells(lib, **kw):
    a = dict(pts=FAKE, pts_elems=40, N=10, cell_units=100, ncx=6, ncy=5, cell_start=FAKE, cell_start_elems=31, status=FAKE, status_elems=1)
    a.update(kw)
    rc = lib.hdy_spatial_cells(a['pts'], a['pts_elems'], a['N'], a['cell_units'], a['ncx'], a['ncy'], a['cell_start'], a['cell_start_elems'], a['status'],
                               a['status_elems'], None)
    return rc, lib.hdy_last_error()


def _neigh(lib, **kw):
    a = dict(pts=FAKE, pts_elems=40, N=10, cell_start=FAKE, cell_start_elems=31, cell_units=100, ncx=6, ncy=5, radii=_radii(10, 50, 100), K=3, C=2,
             counts=FAKE, counts_elems=60, near_d2=FAKE, near_d2_elems=20, near_row=FAKE, near_row_elems=20)
    a.update(kw)
    rc = lib.hdy_spatial_neighbors(a['pts'], a['pts_elems'], a['N'], a['cell_start'], a['cell_start_elems'], a['cell_units'], a['ncx'], a['ncy'],
                                   a['radii'], a['K'], a['C'], a['counts'], a['counts_elems'], a['near_d2'], a['near_d2_elems'], a['near_row'],
                                   a['near_row_elems'], None)
    return rc, lib.hdy_last_error()


def _dens(lib, **kw):
    a = dict(pts=FAKE, pts_elems=40, N=10, g_units=4096, gx=7, gy=3, C=2, grid=FAKE, grid_elems=42)
    a.update(kw)
    rc = lib.hdy_spatial_density(a['pts'], a['pts_elems'], a['N'], a['g_units'], a['gx'], a['gy'], a['C'], a['grid'], a['grid_elems'], None)
    return rc, lib.hdy_last_error()


def _refused(result, word, kw):
    rc, msg = result
    assert rc == _lib.EINVAL and word in msg, (kw, rc, msg)


def test_points_and_grid_checks_are_shared_by_the_entry_points(lib):
    lib.hdy_dispatch_log_reset()
    for call, who in ((_cells, b'spatial_cells'), (_neigh, b'spatial_neighbors'), (_dens, b'spatial_density')):
        _refused(call(lib, pts=None), b'null pts', who)
        for off in (4, 8, 2):
            _refused(call(lib, pts=FAKE + off), b'misaligned pts', who)
        for kw in ({'N': -1, 'pts_elems': -4}, {'pts_elems': -40}):
            _refused(call(lib, **kw), b'negative', kw)
        for n in (39, 41, 0, 10):
            _refused(call(lib, pts_elems=n), b'pts_elems', n)
        assert call(lib, pts=None)[1].startswith(who)
    for call in (_cells, _neigh):
        for kw in ({'cell_units': 0}, {'cell_units': -3}):
            _refused(call(lib, **kw), b'cell_units', kw)
        for kw in ({'ncx': 0}, {'ncy': -1}, {'ncx': 4097, 'ncy': 4096, 'cell_start_elems': 4097 * 4096 + 1},
                   {'ncx': 1 << 24, 'ncy': 2, 'cell_start_elems': (1 << 25) + 1}, {'ncx': 1 << 20, 'ncy': 1 << 20, 'cell_start_elems': 1}):
            _refused(call(lib, **kw), b'at most 16777216 cells', kw)
        assert call(lib, ncx=4096, ncy=4096, cell_start_elems=(1 << 24))[1].find(b'cell_start_elems') >= 0        # the limit itself passes the grid check
        for n in (30, 32, 0, -1):
            _refused(call(lib, cell_start_elems=n), b'cell_start_elems', n)
        _refused(call(lib, cell_start=None), b'null', 'cell_start')
        _refused(call(lib, cell_start=FAKE + 2), b'misaligned', 'cell_start')
    assert _lib.dispatch_log() == []


def test_spatial_cells_argument_checks(lib):
    for n in (0, 2, -1):
        _refused(_cells(lib, status_elems=n), b'status_elems', n)
    _refused(_cells(lib, status=None), b'null', 'status')
    _refused(_cells(lib, status=FAKE + 1), b'misaligned', 'status')


def test_spatial_neighbors_argument_checks(lib):
    for C in (0, -1, 17):
        _refused(_neigh(lib, C=C, counts_elems=30 * C, near_d2_elems=10 * C, near_row_elems=10 * C), b'C=', C)
    for K in (0, -2, 5):
        _refused(_neigh(lib, K=K, radii=_radii(1, 2, 3, 4, 5), counts_elems=20 * K), b'K=', K)
    _refused(_neigh(lib, radii=None), b'null radii', 'radii')
    for r in ((10, 10, 100), (50, 10, 100), (0, 50, 100), (-5, 50, 100), (10, 100, 99)):
        _refused(_neigh(lib, radii=_radii(*r)), b'radii must increase strictly', r)
    _refused(_neigh(lib, radii=_radii(10, 50, 101)), b'passes cell_units=100', 'r_K > cell')
    _refused(_neigh(lib, radii=_radii(101,), K=1, counts_elems=20), b'passes cell_units=100', 'r_K > cell')
    for kw in ({'counts_elems': 59}, {'counts_elems': 61}, {'counts_elems': 0}, {'counts_elems': -60}):
        _refused(_neigh(lib, **kw), b'counts_elems', kw)
    for kw in ({'near_d2_elems': 19}, {'near_d2_elems': 21}, {'near_d2_elems': 0}):
        _refused(_neigh(lib, **kw), b'near_d2_elems', kw)
    for kw in ({'near_row_elems': 19}, {'near_row_elems': 21}, {'near_row_elems': 0}):
        _refused(_neigh(lib, **kw), b'near_row_elems', kw)
    for kw in ({'counts': None}, {'near_d2': None}, {'near_row': None}):
        _refused(_neigh(lib, **kw), b'null', kw)
    for kw in ({'near_d2': FAKE + 4}, {'counts': FAKE + 2}, {'near_row': FAKE + 1}):
        _refused(_neigh(lib, **kw), b'misaligned', kw)
    # the limits themselves pass every check up to the sizes
    _refused(_neigh(lib, C=16, K=4, radii=_radii(1, 2, 3, 100), counts_elems=640, near_d2_elems=160, near_row_elems=1), b'near_row_elems', 'limits')


def test_spatial_density_argument_checks(lib):
    for C in (0, 17):
        _refused(_dens(lib, C=C, grid_elems=21 * C), b'C=', C)
    for g in (0, -16):
        _refused(_dens(lib, g_units=g), b'g_units', g)
    for kw in ({'gx': 0, 'grid_elems': 0}, {'gy': -1}, {'gx': 1 << 16, 'gy': 1 << 15, 'C': 1, 'grid_elems': 1 << 31}, {'gx': 1 << 30, 'gy': 1 << 30}):
        _refused(_dens(lib, **kw), b'fewer than 2^31 entries', kw)
    for n in (41, 43, 0, -42):
        _refused(_dens(lib, grid_elems=n), b'grid_elems', n)
    _refused(_dens(lib, grid=None), b'null grid', 'grid')
    _refused(_dens(lib, grid=FAKE + 2), b'misaligned', 'grid')


def test_zero_points_launch_nothing(lib):
    lib.hdy_dispatch_log_reset()
    z = dict(N=0, pts_elems=0)
    assert _cells(lib, **z)[0] == _lib.OK and _cells(lib, pts=None, cell_start=None, status=None, **z)[0] == _lib.OK
    zn = dict(z, counts_elems=0, near_d2_elems=0, near_row_elems=0)
    assert _neigh(lib, **zn)[0] == _lib.OK and _neigh(lib, pts=None, cell_start=None, counts=None, near_d2=None, near_row=None, **zn)[0] == _lib.OK
    assert _dens(lib, **z)[0] == _lib.OK and _dens(lib, pts=None, grid=None, **z)[0] == _lib.OK
    assert _lib.dispatch_log() == []
    # the sizes and the arithmetic's limits are still checked
    _refused(_cells(lib, cell_start_elems=30, **z), b'cell_start_elems', 'N = 0')
    _refused(_neigh(lib, **dict(zn, counts_elems=6)), b'counts_elems', 'N = 0')
    _refused(_neigh(lib, radii=_radii(10, 5, 100), **zn), b'radii must increase', 'N = 0')
    _refused(_neigh(lib, C=17, **zn), b'C=', 'N = 0')
    _refused(_dens(lib, grid_elems=41, **z), b'grid_elems', 'N = 0')
