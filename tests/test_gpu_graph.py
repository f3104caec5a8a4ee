"""The cell graph on the MI355X (csrc/graph.hip: hdy_graph_knn, hdy_graph_mutual), through ops.spatial_knn / ops.knn_mutual,
hd_yolo_amd/graph.py and evaluation.inference_on_slide(..., measure=True, graph=(k, max_px)).  Every output is compared bit for bit with the
brute-force numpy restatement (tests/graph_ref.py), which tests/test_graph_host.py ties to a double loop, to answers derived by hand and to
a Python restatement of the kernel's ring search.  Every brute-force reference has N <= 3000."""
import contextlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import graph_ref as ref  # noqa: E402
from hd_yolo_amd import _lib, ops  # noqa: E402
from hd_yolo_amd import graph as hgraph  # noqa: E402
from test_gpu_mask_rows import mask_model  # noqa: E402,F401  (the module-scoped fixture)
from test_gpu_slide import synth_u8  # noqa: E402
from test_gpu_spatial import TABLE_KEYS  # noqa: E402

DEV = torch.device('cuda', 0)
R = 64 * ref.UNITS
KS = (1, 3, 8, 16)
POISON32, POISON64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A


@contextlib.contextmanager
def poisoned_empty():
    """torch.empty hands out integer tensors filled with 0x5A bytes: an entry a call leaves unwritten shows"""
    real = torch.empty

    def empty(*a, **k):
        t = real(*a, **k)
        if t.dtype in (torch.int32, torch.int64) and t.numel():
            t.fill_(POISON32 if t.dtype == torch.int32 else POISON64)
        return t

    torch.empty = empty
    try:
        yield
    finally:
        torch.empty = real


def run(xy, cls, k, r, C=3, **kw):
    """ops.spatial_knn on numpy inputs, outputs and workspace pre-filled with 0x5A bytes -> numpy outputs"""
    N = len(xy)
    with poisoned_empty():
        row, d2, count = ops.spatial_knn(torch.from_numpy(xy).to(DEV), k, r, cls=None if cls is None else torch.from_numpy(cls).to(DEV),
                                         C=None if cls is None else C, **kw)
    assert row.dtype == torch.int32 and tuple(row.shape) == (N, k) and d2.dtype == torch.int64 and tuple(d2.shape) == (N, k)
    assert count.dtype == torch.int32 and tuple(count.shape) == (N,)
    return row.cpu().numpy(), d2.cpu().numpy(), count.cpu().numpy()


def same(got, want):
    for g, w, name in zip(got, want, ('nbr_row', 'nbr_d2', 'nbr_count')):
        assert np.array_equal(g, w), (name, np.argwhere(g != w)[:8])


def first(want16, k):
    """the answer for k from the answer for 16: the neighbours are the first k candidates of one order"""
    return want16[0][:, :k].copy(), want16[1][:, :k].copy(), np.minimum(want16[2], k)


def counted(cls, C=3):
    """the classes as ops.spatial_knn(cls=, C=) hands them to the kernel: outside [0, C) a query only"""
    return np.where((cls >= 0) & (cls < C), cls, -1)


@pytest.fixture(scope='module')
def uniform_sets():
    """N -> (xy, the restatement's answer for k = 16): uniform points, every one a node; the small sets within a few radii so that they have
    neighbours, the large ones in 2048 x 2048 px (about nine neighbours within 64 px at N = 3000).  Computed once, never modified."""
    sets = {}
    for N in sorted({1, 2, 63, 257, 3000} | set(KS) | {k + 1 for k in KS}):
        xy, _ = ref.uniform(np.random.default_rng(2000 + N), N, 96 if N <= 17 else 2048)
        sets[N] = (xy, ref.knn(xy, None, 16, R))
    return sets


@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('N', [1, 2, 'k', 'k+1', 63, 257, 3000])
def test_uniform_points(uniform_sets, N, k):
    N = {'k': k, 'k+1': k + 1}.get(N, N)
    xy, want16 = uniform_sets[N]
    want = first(want16, k)
    got = run(xy, None, k, R)
    same(got, want)
    if N == k + 1 and k > 1:
        assert (got[2] > 0).any()
    if N == 3000:
        assert (got[2] == k).any() and (k == 1 or (got[2] < k).any()) and got[1].max() <= R * R


@pytest.mark.parametrize('N', [257, 3000])
def test_the_cell_size_does_not_matter(uniform_sets, N):
    xy, want16 = uniform_sets[N]
    want = first(want16, 8)
    for cell in (R, -(-R // 3), -(-R // 16), 7 * R + 5):
        info = {}
        same(run(xy, None, 8, R, cell_units=cell, info=info), want)
        assert info['cell_units'] == cell and int(info['status']) == 0
    assert -(-R // (-(-R // 17))) == 17
    with pytest.raises(_lib.HdyError, match='17 rings'):
        run(xy, None, 8, R, cell_units=-(-R // 17))


def test_ties_on_a_lattice():
    xy, cls = ref.lattice()
    r = 3 * 8 * ref.UNITS
    want16 = ref.knn(xy, cls, 16, r)
    assert (want16[1][:, :4] == (8 * ref.UNITS) ** 2).sum() > 2000            # many equal distances: the tie rule decides
    for k in (1, 4, 16):
        same(run(xy, cls, k, r), first(want16, k))
    same(run(xy, cls, 4, r, cell_units=8 * ref.UNITS), first(want16, 4))      # every point on a cell border


def test_1500_coincident_points():
    xy = np.full((1500, 2), 12345, dtype=np.int32)
    got = run(xy, None, 16, 1)
    same(got, ref.knn(xy, None, 16, 1))
    assert got[0][0].tolist() == list(range(1, 17)) and got[0][5].tolist() == [0, 1, 2, 3, 4] + list(range(6, 17)) and got[0][1499].tolist() == list(range(16))
    assert not got[1].any() and (got[2] == 16).all()


def test_points_on_cell_borders_corners_and_edges():
    xy, cls = ref.borders(R)
    want = ref.knn(xy, cls, 5, R)
    info = {}
    same(run(xy, cls, 5, R, cell_units=R, info=info), want)
    assert (info['ncx'], info['ncy']) == (5, 4)
    same(run(xy, cls, 5, R, cell_units=R + 1), want)
    same(run(xy, cls, 5, R), want)
    same(run(xy // R, cls, 5, 1, cell_units=1), ref.knn(xy // R, cls, 5, 1))  # cells of one unit, a radius of one unit


def test_a_cluster_in_one_cell_beside_sparse_points():
    """lanes of one wave stop at different rings: the cluster's after ring 1, the sparse points' at the radius"""
    rng = np.random.default_rng(77)
    cell = R // 4
    cluster = (3 * cell + rng.integers(0, cell, (2000, 2))).astype(np.int32)  # all inside cell (3, 3) of the grid of R / 4
    sparse, _ = ref.uniform(rng, 1000)
    xy = np.concatenate([cluster, sparse])[rng.permutation(3000)]
    want = ref.knn(xy, None, 8, R)
    same(run(xy, None, 8, R, cell_units=cell), want)
    same(run(xy, None, 8, R), want)
    same(run(xy, None, 8, R, cell_units=R), want)
    assert (want[1].max(1) > cell * cell).any(), 'no k-th neighbour beyond one cell side'
    assert (want[2] < 8).any(), 'every row has k neighbours'
    assert ((want[2] == 8) & (want[1][:, 7] < 64)).any()                      # and a row whose eight lie within half a pixel


def test_query_only_classes_and_absent_points():
    rng = np.random.default_rng(5)
    xy, cls = ref.mixed(rng)
    assert (cls == -1).any() and (cls == 3).any() and (cls == 2 ** 31 - 1).any() and (xy[:, 0] < 0).any() and (xy[:, 1] < 0).any()
    want = ref.knn(xy, counted(cls), 8, R)
    got = run(xy, cls, 8, R)
    same(got, want)
    absent = (xy < 0).any(1)
    query_only = ~absent & ((cls < 0) | (cls >= 3))
    assert (got[0][absent] == -1).all() and (got[1][absent] == -1).all() and not got[2][absent].any()      # the stated values
    assert got[2][query_only].any()                                                                        # their own rows are computed
    assert not np.isin(got[0], np.nonzero(absent | query_only)[0]).any()                                   # and they are nobody's neighbour
    wide = cls.astype(np.int64)
    wide[wide == 3] = 2 ** 40
    same(run(xy, wide, 8, R), want)
    # without classes every present point is a node
    every = run(xy, None, 8, R)
    same(every, ref.knn(xy, None, 8, R))
    assert np.isin(every[0], np.nonzero(query_only)[0]).any()


def test_coordinates_beyond_the_extent_and_repeats():
    rng = np.random.default_rng(15)
    xy, cls = ref.mixed(rng, 900, 700)
    want = ref.knn(xy, counted(cls), 8, R)
    infos = [{}, {}, {}]
    same(run(xy, cls, 8, R, extent_units=(700 * 16, 700 * 16), info=infos[0]), want)
    same(run(xy, cls, 8, R, extent_units=(300 * 16, 150 * 16), info=infos[1]), want)          # most points fall into the last column / row
    same(run(xy, cls, 8, R, extent_units=(1, 1), cell_units=R, info=infos[2]), want)          # one cell
    assert infos[0]['ncx'] * infos[0]['cell_units'] > xy[:, 0].max() and 2 * infos[1]['ncx'] * infos[1]['cell_units'] < xy[:, 0].max()
    assert 2 * infos[1]['ncy'] * infos[1]['cell_units'] < xy[:, 1].max() and (infos[2]['ncx'], infos[2]['ncy']) == (1, 1)
    a, b = run(xy, cls, 8, R), run(xy, cls, 8, R)
    same(a, b)                                                                                # two runs are bit-identical
    _lib.dispatch_log(reset=True)
    run(xy, cls, 8, R)
    assert _lib.dispatch_log() == ['spatial_cells', 'graph_knn']
    empty = ops.spatial_knn(torch.zeros((0, 2), dtype=torch.int32, device=DEV), 4, R)
    assert [tuple(t.shape) for t in empty] == [(0, 4), (0, 4), (0,)]
    with pytest.raises(_lib.HdyError, match='k=17'):
        run(xy, cls, 17, R)
    with pytest.raises(_lib.HdyError, match='k=0'):
        run(xy, cls, 0, R)
    with pytest.raises(_lib.HdyError, match='max_radius'):
        run(xy, cls, 4, 0)


def test_spatial_neighbors_and_spatial_knn_build_one_cell_index():
    """the same points, cell side and extent: the two calls sort the points into the same cells (ops._cell_index) and launch what they always did"""
    xy, cls = ref.mixed(np.random.default_rng(23), 200, 256)
    assert (xy < 0).any(1).sum() >= 3 and ((cls < 0) | (cls >= 3)).sum() >= 3                 # a few absent, a few out of class
    txy, tcls = torch.from_numpy(xy).to(DEV), torch.from_numpy(cls).to(DEV)
    grid = dict(cell_units=R, extent_units=(256 * ref.UNITS, 256 * ref.UNITS))
    neigh, knn = {}, {}
    _lib.dispatch_log(reset=True)
    ops.spatial_neighbors(txy, tcls, 3, (R // 2, R), info=neigh, **grid)
    got = ops.spatial_knn(txy, 4, R, cls=tcls, C=3, info=knn, **grid)
    assert _lib.dispatch_log() == ['spatial_cells', 'spatial_neighbors', 'spatial_cells', 'graph_knn']
    assert sorted(neigh) == sorted(knn) == ['cell_start', 'cell_units', 'ncx', 'ncy', 'pts', 'status']
    assert torch.equal(neigh['pts'], knn['pts']) and torch.equal(neigh['cell_start'], knn['cell_start'])
    assert (neigh['ncx'], neigh['ncy']) == (knn['ncx'], knn['ncy']) == (4, 4) and neigh['cell_units'] == knn['cell_units'] == R
    assert tuple(knn['pts'].shape) == (200, 4) and tuple(knn['cell_start'].shape) == (17,) and int(knn['cell_start'][-1]) == int((xy >= 0).all(1).sum())
    assert int(neigh['status']) == 0 and int(knn['status']) == 0
    same([t.cpu().numpy() for t in got], ref.knn(xy, counted(cls), 4, R))
    # no points: neither call raises or launches, and the index is the same empty one
    none_xy, none_cls = txy[:0], tcls[:0]
    neigh, knn = {}, {}
    _lib.dispatch_log(reset=True)
    a = ops.spatial_neighbors(none_xy, none_cls, 3, (R // 2, R), info=neigh, **grid)
    b = ops.spatial_knn(none_xy, 4, R, cls=none_cls, C=3, info=knn, **grid)
    assert _lib.dispatch_log() == []
    assert [tuple(t.shape) for t in a] == [(0, 2, 3), (0, 3), (0, 3)] and [tuple(t.shape) for t in b] == [(0, 4), (0, 4), (0,)]
    assert torch.equal(neigh['pts'], knn['pts']) and torch.equal(neigh['cell_start'], knn['cell_start']) and not knn['cell_start'].any()
    assert (neigh['ncx'], neigh['ncy']) == (knn['ncx'], knn['ncy']) == (4, 4)


def test_row_permutation():
    """permuting the rows permutes counts and distances; the rows map through the permutation wherever distances are distinct, and among equal
    distances the lowest NEW row comes first: the permuted call is checked against the restatement on the permuted rows"""
    rng = np.random.default_rng(9)
    for xy, cls, r in (ref.lattice() + (3 * 8 * ref.UNITS,), ref.uniform(rng, 500, 300) + (R,)):
        base = run(xy, cls, 6, r)
        same(base, ref.knn(xy, cls, 6, r))
        perm = rng.permutation(len(xy))
        got = run(xy[perm], cls[perm], 6, r)
        same(got, ref.knn(xy[perm], cls[perm], 6, r))
        assert np.array_equal(got[1], base[1][perm]) and np.array_equal(got[2], base[2][perm])
        held = got[0] >= 0
        there = xy[perm][np.maximum(got[0], 0)].astype(np.int64) - xy[perm][:, None, :].astype(np.int64)
        assert np.array_equal((there ** 2).sum(2)[held], got[1][held])


def test_knn_mutual(uniform_sets):
    def check(nbr_row):
        with poisoned_empty():
            got = ops.knn_mutual(torch.from_numpy(nbr_row).to(DEV))
        assert got.dtype == torch.int32 and tuple(got.shape) == nbr_row.shape
        assert np.array_equal(got.cpu().numpy(), ref.mutual(nbr_row))
        return got.cpu().numpy()

    for N, k in ((2, 1), (17, 16), (257, 3), (3000, 8), (3000, 16)):
        m = check(first(uniform_sets[N][1], k)[0])
    assert m.any() and not m.all()
    xy, cls = ref.mixed(np.random.default_rng(5))
    check(ref.knn(xy, counted(cls), 8, R)[0])
    # any content is memory-safe: -1, N, values far outside, and rows that name themselves
    rng = np.random.default_rng(12)
    wild = rng.integers(-3, 53, (50, 4)).astype(np.int32)
    wild[0] = [2 ** 31 - 1, -2 ** 31, 50, -1]
    wild[1] = [1, 1, 0, 49]
    m = check(wild)
    assert not m[0].any() and m[1, 0] == 1 and m[1, 1] == 1
    _lib.dispatch_log(reset=True)
    ops.knn_mutual(torch.from_numpy(wild).to(DEV))
    assert _lib.dispatch_log() == ['graph_mutual']
    assert tuple(ops.knn_mutual(torch.zeros((0, 4), dtype=torch.int32, device=DEV)).shape) == (0, 4)


def graph_ref_of(xy, cls, k, r):
    row, d2, count = ref.knn(xy, cls, k, r)
    return {'knn_row': row, 'knn_dist': ref.dist(d2), 'knn_count': count, 'knn_mutual': ref.mutual(row).astype(bool)}, d2


def same_graph(g, want, d2, mode='union'):
    for n in ('knn_row', 'knn_dist', 'knn_count', 'knn_mutual'):
        assert g[n].cpu().numpy().dtype == want[n].dtype and np.array_equal(g[n].cpu().numpy(), want[n], equal_nan=True), n
    e = g if 'edge_index' in g else hgraph.edges(g, mode)
    index, ed2, both = ref.edges(want['knn_row'], d2, mode)
    assert e['edge_index'].dtype == torch.int64 and np.array_equal(e['edge_index'].cpu().numpy(), index)
    assert np.array_equal(e['edge_dist'].cpu().numpy(), ref.dist(ed2)) and np.array_equal(e['edge_mutual'].cpu().numpy(), both)
    return index.shape[1]


def test_knn_graph_edges_and_node_features_on_the_device(monkeypatch):
    rng = np.random.default_rng(41)
    N, nc, k = 2000, 3, 6
    px = rng.uniform(0, 900, (N, 2))
    table = {'centroid_x': torch.from_numpy(px[:, 0]).to(DEV), 'centroid_y': torch.from_numpy(px[:, 1]).to(DEV),
             'area': torch.from_numpy(rng.integers(0, 5, N)).to(DEV), 'labels': torch.from_numpy(rng.integers(0, nc + 2, N)).to(DEV)}
    xy = np.where((table['area'].cpu().numpy() > 0)[:, None], np.round(px * 16), -1).astype(np.int32)
    cls = table['labels'].cpu().numpy() - 1
    want, d2 = graph_ref_of(xy, counted(cls, nc), k, 728)
    # with the slide's size nothing is read back: every way a device tensor reaches the host raises
    reads = []

    def guard(name):
        real = getattr(torch.Tensor, name)

        def method(self, *a, **kw):
            if self.is_cuda:
                reads.append(name)
                if reads[0] == 'forbidden':
                    raise AssertionError(f'knn_graph(size=...) read a device tensor back through {name}')
            return real(self, *a, **kw)
        return method

    with monkeypatch.context() as mp:
        for name in ('tolist', 'item', 'cpu', 'numpy', '__bool__', '__int__', '__index__', '__float__'):
            mp.setattr(torch.Tensor, name, guard(name))
        reads.append('forbidden')
        g = hgraph.knn_graph(table, k, 45.5, nc=nc, size=(900, 900))
        reads.clear()
        free = hgraph.knn_graph(table, k, 45.5, nc=nc)                        # without it the extent is read from the points, once
        assert reads == ['tolist']
    assert g['knn_row'].is_cuda and sorted(g) == ['knn_count', 'knn_dist', 'knn_mutual', 'knn_row']
    for mode in ('union', 'mutual', 'directed'):
        E = same_graph(g, want, d2, mode)
        assert E > 0
    assert all(torch.equal(free[n], g[n]) or n == 'knn_dist' for n in g)
    assert np.array_equal(free['knn_dist'].cpu().numpy(), want['knn_dist'], equal_nan=True)
    # node features against a per-row loop
    from test_graph_host import features_ref
    f = hgraph.node_features(g, table['labels'] - 1, nc)
    fw = features_ref(want['knn_row'], d2, cls, nc)
    assert sorted(f) == sorted(fw)
    for n in fw:
        assert f[n].is_cuda and f[n].cpu().numpy().dtype == fw[n].dtype and np.array_equal(f[n].cpu().numpy(), fw[n], equal_nan=True), n
    # without nc every present row is a node, whatever its label
    same_graph(hgraph.knn_graph(table, k, 45.5, size=(900, 900)), *graph_ref_of(xy, None, k, 728))
    none = hgraph.knn_graph({k_: v[:0] for k_, v in table.items()}, 3, 10.0, nc=nc)
    assert tuple(none['knn_row'].shape) == (0, 3) and tuple(hgraph.edges(none)['edge_index'].shape) == (2, 0)


def test_slide_end_to_end(mask_model, tmp_path):
    import evaluation
    _, dep = mask_model
    slide = synth_u8(1024, 7).to(DEV)
    kw = dict(tile=256, overlap=32, batch_size=5, compute_masks=True, label_map=True, measure=True)
    _lib.dispatch_log(reset=True)
    plain = evaluation.inference_on_slide(dep, slide, **kw)['det']
    assert not any(d.startswith('graph') for d in _lib.dispatch_log())
    got = evaluation.inference_on_slide(dep, slide, graph=(4, 64), **kw)['det']
    log = _lib.dispatch_log()
    assert log.count('graph_knn') == 1 and log.count('graph_mutual') == 1
    n = len(plain['boxes'])
    assert n > 5, 'the synthetic mask model found too little on the slide: the test needs detections'
    # a result requested without graph has exactly the keys it has today; with it, one more, and the table keeps its columns
    assert 'graph' not in plain and sorted(plain['nuclei']) == TABLE_KEYS
    assert sorted(got) == sorted(list(plain) + ['graph']) and sorted(got['nuclei']) == TABLE_KEYS
    for key in plain:
        if key != 'nuclei':
            assert torch.equal(got[key], plain[key]), key
    t = got['nuclei']
    for key in TABLE_KEYS:
        assert np.array_equal(t[key].cpu().numpy(), plain['nuclei'][key].cpu().numpy(), equal_nan=t[key].dtype.is_floating_point), key
    nc = dep._model.headers['det'].nc
    # the graph equals the restatement on the table's own centroids
    area = t['area'].cpu().numpy()
    c = np.stack([t['centroid_x'].cpu().numpy(), t['centroid_y'].cpu().numpy()], 1)
    xy = np.where((area > 0)[:, None] & np.isfinite(c), np.round(np.nan_to_num(c) * 16), -1).astype(np.int32)
    cls = t['labels'].cpu().numpy().astype(np.int64) - 1
    want, d2 = graph_ref_of(xy, counted(cls, nc), 4, 64 * 16)
    g = got['graph']
    assert sorted(g) == ['edge_dist', 'edge_index', 'edge_mutual', 'knn_count', 'knn_dist', 'knn_mutual', 'knn_row'] and tuple(g['knn_row'].shape) == (n, 4)
    E = same_graph(g, want, d2, 'union')
    assert E > 0, 'no nucleus of the slide has a neighbour within 64 px: the test needs some'
    # slide_cell_graph on the finished result gives the same, in every mode
    again = evaluation.slide_cell_graph(got, 4, 64, nc=nc)
    assert sorted(again) == sorted(g) and all(np.array_equal(again[key].cpu().numpy(), g[key].cpu().numpy(), equal_nan=True) for key in g)
    same_graph(evaluation.slide_cell_graph(got, 4, 64, nc=nc, mode='mutual'), want, d2, 'mutual')
    # the .npz holds it
    path = str(tmp_path / 'cells.npz')
    evaluation.save_cell_graph(path, g, xy=torch.stack([t['centroid_x'], t['centroid_y']], 1), labels=got['labels'])
    with np.load(path) as z:
        for key in g:
            assert np.array_equal(z[key], g[key].cpu().numpy(), equal_nan=True), key
        assert np.array_equal(z['xy'], c, equal_nan=True) and np.array_equal(z['labels'], got['labels'].cpu().numpy())
    with pytest.raises(ValueError, match='graph needs measure=True'):
        evaluation.inference_on_slide(dep, slide, tile=256, overlap=32, batch_size=5, compute_masks=True, label_map=True, graph=(4, 64))
