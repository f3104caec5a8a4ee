"""Host side of the cell graph (csrc/graph.hip, include/hdyolo_graph.h), no GPU: the brute-force restatement (tests/graph_ref.py) against a
double loop and against answers derived by hand; the kernel's ring traversal and stop rule, restated in Python, against the brute force over
cell sizes from one unit to many radii, clamped grids and a cluster beside sparse points (this is where the stop rule is proved without a
GPU); the extension header and its binding; every invalid call of the two entry points answered by status and message before anything is
dereferenced or launched; and graph.edges / node_features / save_cell_graph on CPU tensors."""
import ctypes
import os

import numpy as np
import pytest
import torch

import graph_ref as ref
from hd_yolo_amd import _header, _lib, build
from hd_yolo_amd import graph as hgraph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 64 * ref.UNITS


def same(got, want):
    for g, w, name in zip(got, want, ('nbr_row', 'nbr_d2', 'nbr_count')):
        assert g.dtype == w.dtype and np.array_equal(g, w), (name, np.argwhere(g != w)[:8])


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [1, 3, 16])
def test_knn_equals_the_double_loop(k):
    rng = np.random.default_rng(k)
    for N, side in ((1, 100), (2, 100), (k, 60), (k + 1, 60), (90, 150), (200, 300)):
        xy, _ = ref.uniform(rng, N, side)
        same(ref.knn(xy, None, k, R, chunk=64), ref.knn_slow(xy, None, k, R))
    xy, cls = ref.mixed(rng, 250, 200)
    got = ref.knn(xy, cls, k, R, chunk=100)
    same(got, ref.knn_slow(xy, cls, k, R))
    absent = (xy < 0).any(1)
    assert absent.any() and (got[0][absent] == -1).all() and (got[1][absent] == -1).all() and not got[2][absent].any()
    assert not np.isin(got[0], np.nonzero(absent | (cls < 0))[0]).any() and got[2][~absent & (cls < 0)].any()
    xy, cls = ref.lattice(9)
    same(ref.knn(xy, cls, k, 3 * 8 * ref.UNITS), ref.knn_slow(xy, cls, k, 3 * 8 * ref.UNITS))


def test_hand_answers():
    # a pair at exactly r: neighbours; at r + 1: not
    row, d2, n = ref.knn(np.array([[5, 7], [5 + R, 7]]), None, 2, R)
    assert row.tolist() == [[1, -1], [0, -1]] and d2.tolist() == [[R * R, -1], [R * R, -1]] and n.tolist() == [1, 1]
    row, d2, n = ref.knn(np.array([[5, 7], [5 + R + 1, 7]]), None, 2, R)
    assert (row == -1).all() and (d2 == -1).all() and n.tolist() == [0, 0]
    # a 3 x 3 lattice of step s, rows 0 .. 8 in reading order: equal distances go to the lowest row
    s = 10
    xy = np.array([[x * s, y * s] for y in range(3) for x in range(3)])
    row, d2, n = ref.knn(xy, None, 4, s)
    assert row[4].tolist() == [1, 3, 5, 7] and d2[4].tolist() == [s * s] * 4 and row[0].tolist() == [1, 3, -1, -1] and n.tolist() == [2, 3, 2, 3, 4, 3, 2, 3, 2]
    row, d2, n = ref.knn(xy, None, 2, 2 * s)
    assert row[4].tolist() == [1, 3] and row[0].tolist() == [1, 3] and row[8].tolist() == [5, 7] and row[2].tolist() == [1, 5]
    row, d2, n = ref.knn(xy, None, 3, 2 * s)
    assert row[0].tolist() == [1, 3, 4] and d2[0].tolist() == [s * s, s * s, 2 * s * s]
    assert ref.knn(xy, None, 1, 2 * s)[0][:, 0].tolist() == [1, 0, 1, 0, 1, 2, 3, 4, 5]
    assert ref.mutual(ref.knn(xy, None, 1, 2 * s)[0])[:, 0].tolist() == [1, 1, 0, 0, 0, 0, 0, 0, 0]
    # three coincident points: the others by row, all at d2 = 0
    xy = np.full((3, 2), 77)
    row, d2, n = ref.knn(xy, None, 2, 1)
    assert row.tolist() == [[1, 2], [0, 2], [0, 1]] and not d2.any() and n.tolist() == [2, 2, 2]
    assert ref.knn(xy, None, 1, 1)[0].tolist() == [[1], [0], [0]]
    assert ref.mutual(row).tolist() == [[1, 1]] * 3 and ref.mutual(ref.knn(xy, None, 1, 1)[0]).tolist() == [[1], [1], [0]]
    # a query-only point in the middle gets neighbours and is nobody's
    row, d2, n = ref.knn(np.array([[0, 0], [3, 0], [6, 0]]), np.array([0, -1, 2 ** 31 - 1]), 2, 10)
    assert row.tolist() == [[2, -1], [0, 2], [0, -1]] and d2.tolist() == [[36, -1], [9, 9], [36, -1]]


# ---- the kernel's traversal and stop rule ---------------------------------------------------------------------------------------------------
def grid_of(xy, cell):
    present = (xy >= 0).all(1)
    mx, my = (int(v) for v in np.where(present[:, None], xy, 0).max(0))
    return mx // cell + 1, my // cell + 1


@pytest.mark.parametrize('k', [1, 4, 16])
@pytest.mark.parametrize('cell', [R, -(-R // 3), -(-R // 16), 7 * R + 5], ids=['r', 'r/3', 'r/16', '7r+5'])
def test_ring_search_equals_knn_whatever_the_cell(k, cell):
    rng = np.random.default_rng(100 + k)
    xy, cls = ref.mixed(rng, 260, 400)
    want = ref.knn(xy, cls, k, R)
    stats = {}
    same(ref.ring_search(xy, cls, k, R, cell, *grid_of(xy, cell), stats=stats), want)
    assert -(-R // cell) <= 16 and stats['last_ring'].max() <= -(-R // cell)
    if cell == -(-R // 16) and k == 16:
        assert stats['last_ring'].max() == 16 and (want[2] < 16).any()       # a row with fewer than k candidates runs all sixteen rings ...
    if cell == -(-R // 16) and k == 1:
        assert 0 < stats['last_ring'][(xy >= 0).all(1)].min() < stats['last_ring'].max() < 16      # ... and the others stop at rings of their own


def test_ring_search_with_cells_of_one_unit():
    rng = np.random.default_rng(7)
    xy = rng.integers(0, 40, (300, 2)).astype(np.int32)                       # many coincident points, every point on a cell border
    for k, r in ((3, 16), (16, 5), (1, 1)):
        same(ref.ring_search(xy, None, k, r, 1, 40, 40), ref.knn(xy, None, k, r))


@pytest.mark.parametrize('grid', [(3, 2), (1, 1), (1, 5), (4, 1)])
def test_ring_search_on_a_grid_smaller_than_the_coordinates(grid):
    """coordinates up to 8 cells, a grid of fewer: everything beyond falls into the last column / row, and the claim of the header (after ring t
    every unvisited point is further than t cells) still holds"""
    rng = np.random.default_rng(11)
    xy, cls = ref.uniform(rng, 300, 8 * 64)
    for k in (2, 8):
        same(ref.ring_search(xy, cls, k, R, R, *grid), ref.knn(xy, cls, k, R))
        same(ref.ring_search(xy, cls, k, R, R // 4 + 1, *grid), ref.knn(xy, cls, k, R))


def test_ring_search_on_a_cluster_beside_sparse_points_and_on_borders():
    rng = np.random.default_rng(13)
    cell = R // 4
    cluster = (3 * cell + rng.integers(0, cell, (200, 2))).astype(np.int32)
    sparse, _ = ref.uniform(rng, 100, 400)
    xy = np.concatenate([cluster, sparse])[rng.permutation(300)]
    stats = {}
    want = ref.knn(xy, None, 8, R)
    same(ref.ring_search(xy, None, 8, R, cell, *grid_of(xy, cell), stats=stats), want)
    assert stats['last_ring'].min() <= 1 and stats['last_ring'].max() == 4 and (want[2] < 8).any()
    assert (want[1].max(1) > cell * cell).any()                              # a k-th neighbour beyond one cell side
    xy, cls = ref.borders(R)
    for cell in (R, R + 1, R // 2):
        same(ref.ring_search(xy, cls, 5, R, cell, *grid_of(xy, cell)), ref.knn(xy, cls, 5, R))


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
    path = os.path.join(ROOT, 'include', 'hdyolo_graph.h')
    ext = _ext.EXTENSIONS['graph']
    assert ext.header == path
    hdr = _header.read(path)
    assert sorted(hdr.functions) == ['hdy_graph_knn', 'hdy_graph_mutual', 'hdy_graph_revision']
    assert not hdr.structs
    assert hdr.constants == {'HDY_GRAPH_REVISION': 1, 'HDY_GRAPH_MAX_K': 16, 'HDY_GRAPH_MAX_RINGS': 16}
    vp, ll, i = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int
    assert hdr.functions['hdy_graph_revision'] == (i, [])
    assert hdr.functions['hdy_graph_knn'] == (i, [vp, ll, i, vp, ll, i, i, i, i, i, vp, ll, vp, ll, vp, ll, vp])
    assert hdr.functions['hdy_graph_mutual'] == (i, [vp, ll, i, i, vp, ll, vp])
    assert [p[0] for p in hdr.params['hdy_graph_knn']] == ['pts', 'pts_elems', 'N', 'cell_start', 'cell_start_elems', 'cell_units', 'ncx', 'ncy', 'k',
                                                           'max_radius', 'nbr_row', 'nbr_row_elems', 'nbr_d2', 'nbr_d2_elems', 'nbr_count',
                                                           'nbr_count_elems', 'stream']
    assert [p[0] for p in hdr.params['hdy_graph_mutual']] == ['nbr_row', 'nbr_row_elems', 'N', 'k', 'mutual', 'mutual_elems', 'stream']
    for name, (res, args) in hdr.functions.items():
        fn = getattr(lib, name)                                            # exported by the built library ...
        assert fn.restype is res and list(fn.argtypes) == args, name      # ... and bound by _ext
        assert name not in _lib.SIGNATURES                                 # the numbered ABI does not know the extension
        assert _ext.SIGNATURES[name] == (res, args) and _ext.PARAMS[name] == hdr.params[name]
    assert (ext.functions, ext.params, ext.constants) == (hdr.functions, hdr.params, hdr.constants)
    assert (ext.revision_fn, ext.revision_macro) == ('hdy_graph_revision', 'HDY_GRAPH_REVISION')
    assert lib.hdy_graph_revision() == ext.revision == 1
    assert _ext.CONSTANTS['HDY_GRAPH_MAX_K'] == 16 and _ext.CONSTANTS['HDY_GRAPH_MAX_RINGS'] == 16
    assert not any(k.startswith('HDY_GRAPH') for k in _lib.CONSTANTS)
    assert 'graph.hip' in build.SOURCES and list(_ext.EXTENSIONS)[3] == 'graph'


def test_graph_knn_shares_the_point_and_grid_checks_of_spatial_neighbors(lib):
    """hdy_graph_knn and hdy_spatial_neighbors answer a bad pts, grid or cell_start with one text, up to the name in front of it (the checks of
    csrc/spatial_common.h), and in the same order when several arguments are bad"""
    lib.hdy_dispatch_log_reset()
    radii = (ctypes.c_int * 3)(10, 50, 100)
    NEIGH = dict(pts=FAKE, pts_elems=40, N=10, cell_start=FAKE, cell_start_elems=13, cell_units=100, ncx=4, ncy=3, radii=radii, K=3, C=2, counts=FAKE,
                 counts_elems=60, near_d2=FAKE, near_d2_elems=20, near_row=FAKE, near_row_elems=20)

    def texts(**kw):
        rc, knn = _knn(lib, **kw)
        assert rc == _lib.EINVAL, kw
        a = dict(NEIGH)
        a.update(kw)
        assert lib.hdy_spatial_neighbors(*(a[n] for n in NEIGH), None) == _lib.EINVAL, kw
        neigh = lib.hdy_last_error()
        assert knn.startswith(b'graph_knn: ') and neigh.startswith(b'spatial_neighbors: '), (knn, neigh)
        return knn[len(b'graph_knn: '):], neigh[len(b'spatial_neighbors: '):]

    cases = [({'pts': None}, b'null pts pointer'), ({'pts': FAKE + 4}, b'misaligned pts pointer (16 bytes)'),
             ({'pts': FAKE + 8}, b'misaligned pts pointer (16 bytes)'),
             ({'N': -1}, b'negative count (N=-1, pts_elems=40)'), ({'pts_elems': -40}, b'negative count (N=10, pts_elems=-40)'),
             ({'pts_elems': 39}, b'pts_elems=39, the call reads 4 * N = 4 * 10'), ({'pts_elems': 44}, b'pts_elems=44, the call reads 4 * N = 4 * 10'),
             ({'cell_units': 0}, b'cell_units=0 must be positive'), ({'cell_units': -3}, b'cell_units=-3 must be positive'),
             ({'ncx': 0}, b'a grid of 0 x 3 cells (sides >= 1, at most 16777216 cells)'),
             ({'ncy': -1}, b'a grid of 4 x -1 cells (sides >= 1, at most 16777216 cells)'),
             ({'ncx': 4097, 'ncy': 4096}, b'a grid of 4097 x 4096 cells (sides >= 1, at most 16777216 cells)'),
             ({'cell_start_elems': 12}, b'cell_start_elems=12, the call reads ncx * ncy + 1 = 13'),
             ({'cell_start_elems': 14}, b'cell_start_elems=14, the call reads ncx * ncy + 1 = 13'),
             ({'cell_start_elems': -1}, b'cell_start_elems=-1, the call reads ncx * ncy + 1 = 13'),
             # several bad arguments: pts before the grid, cell_units before the sides, the grid before cell_start
             ({'pts': None, 'cell_units': 0}, b'null pts pointer'), ({'pts_elems': 39, 'ncx': 0}, b'pts_elems=39, the call reads 4 * N = 4 * 10'),
             ({'N': -1, 'pts': FAKE + 4}, b'negative count (N=-1, pts_elems=40)'), ({'cell_units': 0, 'ncx': 0}, b'cell_units=0 must be positive'),
             ({'ncy': 0, 'cell_start_elems': 5}, b'a grid of 4 x 0 cells (sides >= 1, at most 16777216 cells)')]
    for kw, want in cases:
        knn, neigh = texts(**kw)
        assert knn == neigh == want, (kw, knn, neigh)
    assert _lib.dispatch_log() == []


KNN = dict(pts=FAKE, pts_elems=40, N=10, cell_start=FAKE, cell_start_elems=13, cell_units=100, ncx=4, ncy=3, k=4, max_radius=300, nbr_row=FAKE,
           nbr_row_elems=40, nbr_d2=FAKE, nbr_d2_elems=40, nbr_count=FAKE, nbr_count_elems=10)


def _knn(lib, **kw):
    a = dict(KNN)
    a.update(kw)
    rc = lib.hdy_graph_knn(*(a[n] for n in KNN), None)
    return rc, lib.hdy_last_error()


MUTUAL = dict(nbr_row=FAKE, nbr_row_elems=40, N=10, k=4, mutual=FAKE, mutual_elems=40)


def _mutual(lib, **kw):
    a = dict(MUTUAL)
    a.update(kw)
    rc = lib.hdy_graph_mutual(*(a[n] for n in MUTUAL), None)
    return rc, lib.hdy_last_error()


def test_graph_knn_argument_checks(lib):
    lib.hdy_dispatch_log_reset()
    cases = [({'k': 0}, b'k=0'), ({'k': 17, 'nbr_row_elems': 170, 'nbr_d2_elems': 170}, b'k=17'), ({'k': -1}, b'k=-1'),
             ({'max_radius': 0}, b'max_radius'), ({'max_radius': -5}, b'max_radius'),
             ({'max_radius': 1601}, b'17 rings'), ({'max_radius': 17, 'cell_units': 1}, b'17 rings'), ({'max_radius': 2 ** 31 - 1}, b'rings'),
             ({'cell_units': 0}, b'cell_units'), ({'ncx': 0}, b'cells'), ({'ncy': -1}, b'cells'), ({'ncx': 1 << 13, 'ncy': (1 << 11) + 1}, b'cells'),
             ({'N': -1}, b'negative'), ({'pts_elems': -40}, b'negative'),
             ({'pts_elems': 39}, b'pts_elems'), ({'pts_elems': 41}, b'pts_elems'),
             ({'cell_start_elems': 12}, b'cell_start_elems'), ({'cell_start_elems': 14}, b'cell_start_elems'),
             ({'nbr_row_elems': 39}, b'nbr_row_elems'), ({'nbr_row_elems': 41}, b'nbr_row_elems'),
             ({'nbr_d2_elems': 39}, b'nbr_d2_elems'), ({'nbr_d2_elems': 41}, b'nbr_d2_elems'),
             ({'nbr_count_elems': 9}, b'nbr_count_elems'), ({'nbr_count_elems': 11}, b'nbr_count_elems'),
             ({'pts': FAKE + 8}, b'misaligned'), ({'pts': FAKE + 4}, b'misaligned'), ({'nbr_d2': FAKE + 4}, b'misaligned'),
             ({'cell_start': FAKE + 2}, b'misaligned'), ({'nbr_row': FAKE + 1}, b'misaligned'), ({'nbr_count': FAKE + 3}, b'misaligned'),
             ({'pts': None}, b'null'), ({'cell_start': None}, b'null'), ({'nbr_row': None}, b'null'), ({'nbr_d2': None}, b'null'),
             ({'nbr_count': None}, b'null')]
    for kw, word in cases:
        rc, msg = _knn(lib, **kw)
        assert rc == _lib.EINVAL and word in msg, (kw, msg)
    # sixteen rings exactly pass the ring check (and fail the next one the case breaks)
    rc, msg = _knn(lib, max_radius=1600, nbr_count_elems=9)
    assert rc == _lib.EINVAL and b'nbr_count_elems' in msg
    empty = dict(N=0, pts_elems=0, nbr_row_elems=0, nbr_d2_elems=0, nbr_count_elems=0)
    assert _knn(lib, pts=None, cell_start=None, nbr_row=None, nbr_d2=None, nbr_count=None, **empty)[0] == _lib.OK          # N = 0 launches nothing
    assert _knn(lib, **dict(empty, nbr_count_elems=1))[0] == _lib.EINVAL                                                    # the sizes are still checked
    assert _knn(lib, **dict(empty, k=0))[0] == _lib.EINVAL
    assert _lib.dispatch_log() == []


def test_graph_mutual_argument_checks(lib):
    lib.hdy_dispatch_log_reset()
    cases = [({'k': 0, 'nbr_row_elems': 0, 'mutual_elems': 0}, b'k=0'), ({'k': 17, 'nbr_row_elems': 170, 'mutual_elems': 170}, b'k=17'),
             ({'N': -1}, b'negative'), ({'nbr_row_elems': 39}, b'nbr_row_elems'), ({'nbr_row_elems': 41}, b'nbr_row_elems'),
             ({'mutual_elems': 39}, b'mutual_elems'), ({'mutual_elems': 41}, b'mutual_elems'),
             ({'nbr_row': FAKE + 2}, b'misaligned'), ({'mutual': FAKE + 1}, b'misaligned'), ({'nbr_row': None}, b'null'), ({'mutual': None}, b'null')]
    for kw, word in cases:
        rc, msg = _mutual(lib, **kw)
        assert rc == _lib.EINVAL and word in msg, (kw, msg)
    assert _mutual(lib, N=0, nbr_row_elems=0, mutual_elems=0, nbr_row=None, mutual=None)[0] == _lib.OK
    assert _mutual(lib, N=0, nbr_row_elems=0, mutual_elems=4)[0] == _lib.EINVAL
    assert _lib.dispatch_log() == []


def test_the_default_cell_is_host_arithmetic_within_its_floors():
    from hd_yolo_amd import ops
    side = 2048 * 16
    cell = ops.knn_cell_units(100000, 8, 64 * 16, side - 1, side - 1)
    assert abs(cell * cell * 100000 / (side * side) - ops.KNN_CELL_FILL * 8) < 1.0       # about KNN_CELL_FILL * k points per cell
    assert ops.knn_cell_units(10 ** 6, 1, 16 * 4096, side - 1, side - 1) == 4096          # ceil(max_radius / 16 rings)
    assert ops.knn_cell_units(10 ** 9, 1, 16, (1 << 26) - 1, 5) == (1 << 26) // ops.SPATIAL_GRID_SIDE
    assert ops.knn_cell_units(0, 8, 1, 0, 0, fill=2) == 4 and ops.knn_cell_units(5, 1, 1, 0, 0) == 1


# ---- graph.py on CPU tensors ----------------------------------------------------------------------------------------------------------------
def graph_of(nbr_row, nbr_d2, nbr_count):
    return {'knn_row': torch.from_numpy(nbr_row), 'knn_dist': torch.from_numpy(ref.dist(nbr_d2)), 'knn_count': torch.from_numpy(nbr_count),
            'knn_mutual': torch.from_numpy(ref.mutual(nbr_row).astype(bool))}


def features_ref(nbr_row, nbr_d2, cls, nc):
    N, k = nbr_row.shape
    d = ref.dist(nbr_d2)
    out = {n: np.full(N, np.nan) for n in ('knn_mean_dist', 'knn_min_dist', 'knn_max_dist')}
    out['in_degree'] = np.zeros(N, dtype=np.int32)
    out['knn_class_counts'] = np.zeros((N, nc), dtype=np.int32)
    for p in range(N):
        held = [s for s in range(k) if nbr_row[p, s] >= 0]
        total = 0.0
        for s in held:
            total += d[p, s]
            out['in_degree'][nbr_row[p, s]] += 1
            if 0 <= cls[nbr_row[p, s]] < nc:
                out['knn_class_counts'][p, cls[nbr_row[p, s]]] += 1
        if held:
            out['knn_mean_dist'][p], out['knn_min_dist'][p], out['knn_max_dist'][p] = total / len(held), d[p, held].min(), d[p, held].max()
    return out


@pytest.mark.parametrize('k,r', [(1, R), (4, 20 * 16), (8, R)])
def test_edges_and_node_features_on_cpu_tensors(k, r):
    rng = np.random.default_rng(k)
    xy, cls = ref.mixed(rng, 300, 400)
    knn = ref.knn(xy, cls, k, r)
    assert (knn[0] < 0).any() and (knn[0] >= 0).any()                         # padding slots beside held ones
    g = graph_of(*knn)
    sizes = {}
    for mode in ('union', 'mutual', 'directed'):
        e = hgraph.edges(g, mode)
        index, d2, both = ref.edges(knn[0], knn[1], mode)
        assert e['edge_index'].dtype == torch.int64 and e['edge_dist'].dtype == torch.float64 and e['edge_mutual'].dtype == torch.bool
        assert np.array_equal(e['edge_index'].numpy(), index) and np.array_equal(e['edge_dist'].numpy(), ref.dist(d2)) and np.array_equal(e['edge_mutual'].numpy(), both)
        sizes[mode] = index.shape[1]
        if mode != 'directed':
            assert (index[0] < index[1]).all() and (np.diff(index[0] * 300 + index[1]) > 0).all()
    assert sizes['directed'] == int(knn[2].sum()) == sizes['union'] + sizes['mutual'] and sizes['mutual'] > 0
    f = hgraph.node_features(g, torch.from_numpy(cls), 3)
    want = features_ref(knn[0], knn[1], cls, 3)
    assert sorted(f) == sorted(want)
    for n in want:
        assert f[n].numpy().dtype == want[n].dtype and np.array_equal(f[n].numpy(), want[n], equal_nan=True), n
    assert sorted(hgraph.node_features(g)) == ['in_degree', 'knn_max_dist', 'knn_mean_dist', 'knn_min_dist']
    with pytest.raises(ValueError, match='mode'):
        hgraph.edges(g, 'delaunay')


def test_empty_graphs():
    for N in (0, 5):                                                          # no rows; rows without any neighbour
        xy = np.arange(2 * N).reshape(N, 2) * 10000
        g = graph_of(*ref.knn(xy, None, 3, 50))
        for mode in ('union', 'mutual', 'directed'):
            e = hgraph.edges(g, mode)
            assert tuple(e['edge_index'].shape) == (2, 0) and tuple(e['edge_dist'].shape) == (0,) and tuple(e['edge_mutual'].shape) == (0,)
        f = hgraph.node_features(g, torch.zeros(N, dtype=torch.int64), 2)
        assert tuple(f['knn_class_counts'].shape) == (N, 2) and not f['in_degree'].any() and bool(torch.isnan(f['knn_mean_dist']).all())
        assert tuple(f['knn_min_dist'].shape) == (N,) and bool(torch.isnan(f['knn_max_dist']).all())


def test_save_cell_graph_round_trips(tmp_path):
    rng = np.random.default_rng(3)
    xy, cls = ref.mixed(rng, 120, 200)
    g = graph_of(*ref.knn(xy, cls, 4, R))
    e = hgraph.edges(g, 'union')
    path = str(tmp_path / 'cells.npz')
    hgraph.save_cell_graph(path, g, e, xy=torch.from_numpy(xy), labels=torch.from_numpy(cls) + 1)
    with np.load(path) as z:
        assert sorted(z.files) == sorted(hgraph.GRAPH_KEYS + hgraph.EDGE_KEYS + ('xy', 'labels'))
        for n in hgraph.GRAPH_KEYS:
            assert z[n].dtype == g[n].numpy().dtype and np.array_equal(z[n], g[n].numpy(), equal_nan=True), n
        for n in hgraph.EDGE_KEYS:
            assert z[n].dtype == e[n].numpy().dtype and np.array_equal(z[n], e[n].numpy()), n
        assert np.array_equal(z['xy'], xy) and np.array_equal(z['labels'], cls + 1)
    hgraph.save_cell_graph(path, g, e)
    with np.load(path) as z:
        assert sorted(z.files) == sorted(hgraph.GRAPH_KEYS + hgraph.EDGE_KEYS)
    with pytest.raises(ValueError, match='npz'):
        hgraph.save_cell_graph(str(tmp_path / 'cells.csv'), g, e)
