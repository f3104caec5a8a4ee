"""The neighbourhood features on the MI355X (csrc/spatial.hip: hdy_spatial_cells, hdy_spatial_neighbors, hdy_spatial_density), through
ops.spatial_neighbors / ops.spatial_density, hd_yolo_amd/spatial.py and evaluation.inference_on_slide(..., measure=True, neighbors=...).
Every output is compared bit for bit with the brute-force numpy restatement (tests/spatial_ref.py), which tests/test_spatial_host.py ties to a
double loop and to answers derived by hand."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import spatial_ref as ref  # noqa: E402
from hd_yolo_amd import _lib, ops, spatial  # noqa: E402
from test_gpu_mask_rows import mask_model  # noqa: E402,F401  (the module-scoped fixture)
from test_gpu_slide import synth_u8  # noqa: E402

DEV = torch.device('cuda', 0)
RK = ref.RADII[-1]


def run(xy, cls, C, radii, cell_units=None, info=None):
    """ops.spatial_neighbors on numpy inputs -> numpy outputs"""
    N, K = len(xy), len(radii)
    counts, d2, row = ops.spatial_neighbors(torch.from_numpy(xy).to(DEV), torch.from_numpy(cls).to(DEV), C, radii, cell_units=cell_units, info=info)
    assert counts.dtype == torch.int32 and tuple(counts.shape) == (N, K, C)
    assert d2.dtype == torch.int64 and tuple(d2.shape) == (N, C) and row.dtype == torch.int32 and tuple(row.shape) == (N, C)
    return counts.cpu().numpy(), d2.cpu().numpy(), row.cpu().numpy()


def same(got, want):
    for g, w, name in zip(got, want, ('counts', 'near_d2', 'near_row')):
        assert np.array_equal(g, w), (name, np.argwhere(g != w)[:8])


def check(xy, cls, C, radii, cell_units=None, want=None):
    got = run(xy, cls, C, radii, cell_units)
    same(got, ref.neighbors(xy, cls, C, radii) if want is None else want)
    return got


@pytest.fixture(scope='module')
def uniform_sets():
    """N -> (xy, cls, the restatement's answer) for points uniform in 2048 x 2048 px, C = 3, radii 16 / 32 / 64 px: computed once, never modified"""
    sets = {}
    for N in (1, 2, 63, 257, 3000):
        xy, cls = ref.uniform(np.random.default_rng(1000 + N), N)
        if N == 2:
            xy[1] = xy[0] + np.array([ref.RADII[0], 0], dtype=np.int32)         # the pair at exactly r_1
        sets[N] = (xy, cls, ref.neighbors(xy, cls, 3, ref.RADII))
    return sets


@pytest.mark.parametrize('N', [1, 2, 63, 257, 3000])
def test_uniform_points(uniform_sets, N):
    xy, cls, want = uniform_sets[N]
    got = check(xy, cls, 3, ref.RADII, want=want)
    if N == 2:
        assert got[0][:, 0].sum() == 2 and got[1].max() == ref.RADII[0] ** 2
    if N == 3000:
        assert got[0][:, 2].sum() > 3000 and (got[2] >= 0).any() and (got[2] < 0).any()


@pytest.mark.parametrize('N', [63, 257, 3000])
def test_the_cell_size_does_not_matter(uniform_sets, N):
    xy, cls, want = uniform_sets[N]
    for cell in (RK, 2 * RK, 7 * RK + 5):
        info = {}
        same(run(xy, cls, 3, ref.RADII, cell_units=cell, info=info), want)
        assert info['cell_units'] == cell and int(info['status']) == 0
    with pytest.raises(_lib.HdyError, match='passes cell_units'):
        run(xy, cls, 3, ref.RADII, cell_units=RK - 1)


def test_points_on_cell_borders_corners_and_edges():
    """every border of a 5 x 4 grid of cells of r_K units, one unit to either side, coordinate 0 and the largest coordinate of the grid: the
    queries of the corner and edge cells clip their nine cells, and pairs at exactly r_K sit in neighbouring cells"""
    xy, cls = ref.borders(RK)
    assert xy.min() == 0 and xy[:, 0].max() == 5 * RK - 1 and xy[:, 1].max() == 4 * RK - 1
    assert {0, RK - 1, RK, RK + 1} <= set(xy[:, 0].tolist())                    # pairs at exactly r_K, and one unit to either side of it
    want = ref.neighbors(xy, cls, 3, ref.RADII)
    info = {}
    same(run(xy, cls, 3, ref.RADII, cell_units=RK, info=info), want)
    assert (info['ncx'], info['ncy']) == (5, 4)
    same(run(xy, cls, 3, ref.RADII), want)
    same(run(xy, cls, 3, ref.RADII, cell_units=RK + 1), want)
    # one radius of one unit: only coincident or adjacent points
    check(xy, cls, 3, (1,), cell_units=RK)
    check(xy // RK, cls, 3, (1,), cell_units=1)                               # cells of one unit: every point sits on a border


def test_1500_coincident_points():
    xy = np.full((1500, 2), 12345, dtype=np.int32)
    cls = (np.arange(1500) % 3).astype(np.int32)
    got = check(xy, cls, 3, ref.RADII)
    assert got[0][0].tolist() == [[499, 500, 500]] * 3 and got[1].max() == 0 and got[2][0].tolist() == [3, 1, 2] and got[2][3].tolist() == [0, 1, 2]


def test_a_cluster_in_one_cell_beside_sparse_points():
    rng = np.random.default_rng(77)
    cluster = (3 * RK + rng.integers(0, RK, (2000, 2))).astype(np.int32)      # all inside cell (3, 3) of the r_K grid
    sparse, _ = ref.uniform(rng, 1000)
    xy = np.concatenate([cluster, sparse])[rng.permutation(3000)]
    cls = rng.integers(0, 3, 3000).astype(np.int32)
    want = ref.neighbors(xy, cls, 3, ref.RADII)
    same(run(xy, cls, 3, ref.RADII, cell_units=RK), want)
    same(run(xy, cls, 3, ref.RADII), want)
    assert want[0].max() > 300


def test_query_only_classes_and_absent_points():
    rng = np.random.default_rng(5)
    xy, cls = ref.mixed(rng)
    assert (cls == -1).any() and (cls == 3).any() and (cls == 2 ** 31 - 1).any() and (xy[:, 0] < 0).any() and (xy[:, 1] < 0).any()
    got = check(xy, cls, 3, ref.RADII)
    absent = (xy < 0).any(1)
    query_only = ~absent & ((cls < 0) | (cls >= 3))
    assert not got[0][absent].any() and (got[1][absent] == -1).all() and (got[2][absent] == -1).all()       # the stated values
    assert got[0][query_only].any()                                                                          # their own rows are computed
    assert not np.isin(got[2], np.nonzero(absent | query_only)[0]).any()                                     # and they are nobody's neighbour
    # the same classes as int64, beyond the int32 range too
    wide = cls.astype(np.int64)
    wide[wide == 3] = 2 ** 40
    same(run(xy, wide, 3, ref.RADII), got)
    # counted points alone give the same counts to everybody
    keep = ~(absent | query_only)
    alone = ref.neighbors(xy[keep], cls[keep], 3, ref.RADII)
    assert np.array_equal(alone[0], got[0][keep]) and np.array_equal(alone[1], got[1][keep])


@pytest.mark.parametrize('C,K', [(16, 4), (1, 1)])
def test_the_limits_of_classes_and_radii(C, K):
    rng = np.random.default_rng(C * 10 + K)
    xy, _ = ref.uniform(rng, 600, 256)
    cls = rng.integers(-1, C + 1, 600).astype(np.int32)
    radii = (5 * 16, 11 * 16, 20 * 16 + 3, 33 * 16)[:K]
    got = check(xy, cls, C, radii)
    assert got[0][:, K - 1].sum() > 0 and (got[2] >= 0).any()
    with pytest.raises(_lib.HdyError, match='C='):
        run(xy, cls, 17, radii)
    with pytest.raises(_lib.HdyError, match='K='):
        run(xy, cls, C, (1, 2, 3, 4, 5))
    with pytest.raises(_lib.HdyError, match='radii must increase'):
        run(xy, cls, C, (7, 7) if K > 1 else (0,))


def test_row_permutation_on_a_lattice():
    """permuting the rows permutes counts and near_d2 and maps near_row through the permutation, except that among equal distances the LOWEST
    ROW wins, which after the permutation is another point: so the permuted call is checked against the restatement on the permuted rows, and
    the distances against the unpermuted call"""
    xy, cls = ref.lattice()
    radii = (8 * 16, 16 * 16, 24 * 16)
    base = check(xy, cls, 3, radii)
    assert (base[1] == (8 * 16) ** 2).sum() > 500                              # many equal distances: the tie rule decides
    perm = np.random.default_rng(9).permutation(len(xy))
    got = check(xy[perm], cls[perm], 3, radii)
    assert np.array_equal(got[0], base[0][perm]) and np.array_equal(got[1], base[1][perm])
    # near_row points at a point at the same distance and of the same class as the unpermuted answer's, the lowest new row among those
    old_of_new = perm
    hit = got[2] >= 0
    assert np.array_equal(hit, base[2][perm] >= 0)
    q, c = np.nonzero(hit)
    there = xy[old_of_new[got[2][q, c]]].astype(np.int64) - xy[perm][q].astype(np.int64)
    assert np.array_equal((there ** 2).sum(1), got[1][q, c]) and np.array_equal(cls[old_of_new[got[2][q, c]]], c)
    # distinct distances: no ties, so near_row maps through the permutation exactly
    rng = np.random.default_rng(10)
    xy2, cls2 = ref.uniform(rng, 500, 300)
    b2 = check(xy2, cls2, 3, ref.RADII)
    perm2 = rng.permutation(500)
    g2 = check(xy2[perm2], cls2[perm2], 3, ref.RADII)
    new_of_old = np.empty(500, dtype=np.int64)
    new_of_old[perm2] = np.arange(500)
    mapped = np.where(b2[2][perm2] >= 0, new_of_old[np.maximum(b2[2][perm2], 0)], -1)
    ties = g2[2] != mapped                                                     # the few exact ties of a random set: the lowest row is another point
    assert np.array_equal(g2[1][ties], b2[1][perm2][ties])
    assert np.array_equal(g2[0], b2[0][perm2]) and np.array_equal(g2[1], b2[1][perm2]) and np.array_equal(g2[2][~ties], mapped[~ties]) and ties.mean() < 0.05


def test_poisoned_outputs_and_workspace_and_repeats(monkeypatch):
    """the calls write every entry of their outputs and of their workspace themselves (torch.empty is made to hand out poison), and two repeats are
    bit-identical"""
    rng = np.random.default_rng(3)
    xy, cls = ref.mixed(rng, 900, 700)
    want = ref.neighbors(xy, cls, 3, ref.RADII)
    real_empty = torch.empty
    poison = -0x5A5A5A5B

    def poisoned(*a, **k):
        t = real_empty(*a, **k)
        if t.dtype in (torch.int64, torch.int32):
            t.fill_(poison)
        return t

    runs, infos = [], []
    for _ in range(2):
        with monkeypatch.context() as mp:
            mp.setattr(torch, 'empty', poisoned)
            infos.append({})
            runs.append(run(xy, cls, 3, ref.RADII, info=infos[-1]))
            grid = ops.spatial_density(torch.from_numpy(xy).to(DEV), torch.from_numpy(cls).to(DEV), 3, 4096, 2, 3)
    same(runs[0], want)
    same(runs[1], runs[0])
    assert not any((r == poison).any() for r in runs[0])
    assert np.array_equal(grid.cpu().numpy(), ref.density(xy, cls, 3, 4096, 2, 3))
    for info in infos:
        start = info['cell_start'].cpu().numpy()
        assert len(start) == info['ncx'] * info['ncy'] + 1 and start[0] == 0 and (np.diff(start) >= 0).all()
        assert start[-1] == int(((xy >= 0).all(1)).sum()) and int(info['status']) == 0
    assert np.array_equal(infos[0]['cell_start'].cpu().numpy(), infos[1]['cell_start'].cpu().numpy())
    _lib.dispatch_log(reset=True)
    run(xy, cls, 3, ref.RADII)
    assert _lib.dispatch_log() == ['spatial_cells', 'spatial_neighbors']
    empty = ops.spatial_neighbors(torch.zeros((0, 2), dtype=torch.int32, device=DEV), torch.zeros((0,), dtype=torch.int32, device=DEV), 3, ref.RADII)
    assert [tuple(t.shape) for t in empty] == [(0, 3, 3), (0, 3), (0, 3)]


def test_cells_status_word_and_cell_start():
    rng = np.random.default_rng(21)
    xy, cls = ref.mixed(rng, 400, 600)
    info = {}
    run(xy, cls, 3, ref.RADII, info=info)
    pts, cell, ncx, ncy = info['pts'], info['cell_units'], info['ncx'], info['ncy']
    host = pts.cpu().numpy()
    present = (host[:, :2] >= 0).all(1)
    P = int(present.sum())
    assert present[:P].all() and not present[P:].any() and sorted(host[:, 3].tolist()) == list(range(400))         # absent points last, every row once
    cid = (host[:P, 1] // cell) * ncx + host[:P, 0] // cell
    assert (np.diff(cid) >= 0).all()
    start, status = ops.spatial_cells(pts, cell, ncx, ncy)
    assert int(status) == 0
    assert np.array_equal(start.cpu().numpy(), np.searchsorted(cid, np.arange(ncx * ncy + 1), side='left'))
    # two points of different cells exchanged: bit 0; a present point behind an absent one: bit 0; every entry stays inside [0, N]
    a, b = 0, P - 1
    assert cid[a] != cid[b]
    for swap in ((a, b), (P - 1, P)):
        broken = pts.clone()
        broken[list(swap)] = pts[list(swap[::-1])]
        start, status = ops.spatial_cells(broken, cell, ncx, ncy)
        assert int(status) & 1, swap
        s = start.cpu().numpy()
        assert s.min() >= 0 and s.max() <= 400
    # the order inside a cell is free: reversed runs of equal cells are still in cell order, and the answer is the same
    order = np.lexsort((-np.arange(P), cid))
    again = torch.cat([pts[:P][torch.from_numpy(order).to(DEV)], pts[P:]]).contiguous()
    start2, status2 = ops.spatial_cells(again, cell, ncx, ncy)
    assert int(status2) == 0 and torch.equal(start2, ops.spatial_cells(pts, cell, ncx, ncy)[0])
    got = ops.spatial_neighbors_sorted(again, start2, cell, ncx, ncy, ref.RADII, 3)
    same([t.cpu().numpy() for t in got], ref.neighbors(xy, cls, 3, ref.RADII))


def test_density_against_add_at():
    rng = np.random.default_rng(31)
    xy, cls = ref.mixed(rng, 5000, 1000)
    g = 256 * 16
    for gx, gy, C in ((4, 4, 3), (3, 2, 3), (1, 1, 1), (5, 7, 16)):                # 1000 px = 3.9 fields: (3, 2) and (1, 1) leave points outside
        got = ops.spatial_density(torch.from_numpy(xy).to(DEV), torch.from_numpy(cls).to(DEV), C, g, gx, gy)
        assert got.dtype == torch.int32 and tuple(got.shape) == (gy, gx, C)
        want = ref.density(xy, cls, C, g, gx, gy)
        assert np.array_equal(got.cpu().numpy(), want)
    full = ref.density(xy, cls, 3, g, 4, 4)
    assert full.sum() == int(((xy >= 0).all(1) & (cls >= 0) & (cls < 3)).sum()) and ref.density(xy, cls, 3, g, 3, 2).sum() < full.sum()
    _lib.dispatch_log(reset=True)
    ops.spatial_density(torch.from_numpy(xy).to(DEV), torch.from_numpy(cls).to(DEV), 3, g, 4, 4)
    assert _lib.dispatch_log() == ['spatial_density']
    none = ops.spatial_density(torch.zeros((0, 2), dtype=torch.int32, device=DEV), torch.zeros((0,), dtype=torch.int32, device=DEV), 2, g, 3, 2)
    assert tuple(none.shape) == (2, 3, 2) and not bool(none.any())


def test_neighborhood_and_interaction_matrix_on_the_device():
    rng = np.random.default_rng(41)
    N, nc = 2000, 3
    px = rng.uniform(0, 900, (N, 2))
    table = {'centroid_x': torch.from_numpy(px[:, 0]).to(DEV), 'centroid_y': torch.from_numpy(px[:, 1]).to(DEV),
             'area': torch.from_numpy(rng.integers(0, 5, N)).to(DEV), 'labels': torch.from_numpy(rng.integers(0, nc + 2, N)).to(DEV)}
    out = spatial.neighborhood(table, nc, (30, 45.5), field_px=256, size=(900, 900))
    xy = np.where((table['area'].cpu().numpy() > 0)[:, None], np.round(px * 16), -1).astype(np.int32)
    cls = table['labels'].cpu().numpy() - 1
    counts, d2, row = ref.neighbors(xy, cls, nc, (480, 728))
    assert np.array_equal(out['neighbors'].cpu().numpy(), counts) and np.array_equal(out['nearest_row'].cpu().numpy(), row)
    dist = np.where(d2 < 0, np.nan, np.sqrt(np.maximum(d2, 0).astype(np.float64)) / 16)
    assert out['nearest_dist'].dtype == torch.float64 and np.array_equal(out['nearest_dist'].cpu().numpy(), dist, equal_nan=True)
    assert np.array_equal(out['density'].cpu().numpy(), ref.density(xy, cls, nc, 4096, 4, 4))
    m = spatial.interaction_matrix(out['neighbors'], table['labels'] - 1, nc)
    assert m.is_cuda and np.array_equal(m.cpu().numpy(), ref.interaction(counts, cls, nc))
    # without the slide's size the extent is read from the points: the same columns
    free = spatial.neighborhood(table, nc, (30, 45.5))
    assert sorted(free) == ['nearest_dist', 'nearest_row', 'neighbors'] and torch.equal(free['neighbors'], out['neighbors'])


TABLE_KEYS = ['area', 'bbox', 'border_edges', 'centroid_x', 'centroid_y', 'compactness', 'eccentricity', 'equivalent_diameter', 'labels', 'major_axis',
              'mean_rgb', 'minor_axis', 'orientation', 'perimeter_edges', 'scores', 'std_rgb', 'touches_border']


def test_slide_end_to_end(mask_model, tmp_path):
    import evaluation
    _, dep = mask_model
    slide = synth_u8(1024, 7).to(DEV)
    kw = dict(tile=256, overlap=32, batch_size=5, compute_masks=True, label_map=True, measure=True)
    _lib.dispatch_log(reset=True)
    plain = evaluation.inference_on_slide(dep, slide, **kw)['det']
    assert not any(d.startswith('spatial') for d in _lib.dispatch_log())
    got = evaluation.inference_on_slide(dep, slide, neighbors=(32, 64), **kw)['det']
    assert _lib.dispatch_log().count('spatial_neighbors') == 1
    n = len(plain['boxes'])
    assert n > 1, 'the synthetic mask model found too little on the slide: the test needs detections'
    # a result requested without neighbors has exactly the keys it has today
    assert 'nuclei' in plain and sorted(plain['nuclei']) == TABLE_KEYS
    assert sorted(got) == sorted(plain) and sorted(got['nuclei']) == sorted(TABLE_KEYS + ['neighbors', 'nearest_dist', 'nearest_row'])
    for k in plain:
        if k != 'nuclei':
            assert torch.equal(got[k], plain[k]), k
    t = got['nuclei']
    for k in TABLE_KEYS:
        assert torch.equal(t[k], plain['nuclei'][k]) or t[k].dtype.is_floating_point and np.array_equal(t[k].cpu().numpy(), plain['nuclei'][k].cpu().numpy(), equal_nan=True), k
    nc = dep._model.headers['det'].nc
    # the new columns equal the restatement on the table's own centroids
    area = t['area'].cpu().numpy()
    c = np.stack([t['centroid_x'].cpu().numpy(), t['centroid_y'].cpu().numpy()], 1)
    xy = np.where((area > 0)[:, None] & np.isfinite(c), np.round(np.nan_to_num(c) * 16), -1).astype(np.int32)
    cls = t['labels'].cpu().numpy().astype(np.int64) - 1
    counts, d2, row = ref.neighbors(xy, cls, nc, (32 * 16, 64 * 16))
    assert tuple(t['neighbors'].shape) == (n, 2, nc) and np.array_equal(t['neighbors'].cpu().numpy(), counts)
    assert np.array_equal(t['nearest_row'].cpu().numpy(), row)
    assert np.array_equal(t['nearest_dist'].cpu().numpy(), np.where(d2 < 0, np.nan, np.sqrt(np.maximum(d2, 0).astype(np.float64)) / 16), equal_nan=True)
    assert counts.sum() > 0, 'no nucleus of the slide has a neighbour within 64 px: the test needs some'
    # slide_neighborhood on the finished result gives the same columns, and a density grid of 256 px fields
    nb = evaluation.slide_neighborhood(got, nc, (32, 64), field_px=256)
    assert torch.equal(nb['neighbors'], t['neighbors']) and tuple(nb['density'].shape) == (4, 4, nc)
    assert np.array_equal(nb['density'].cpu().numpy(), ref.density(xy, cls, nc, 4096, 4, 4))
    # save_nucleus_table writes the new columns unchanged
    path = str(tmp_path / 'nuclei.npz')
    evaluation.save_nucleus_table(path, t)
    with np.load(path) as z:
        assert np.array_equal(z['neighbors'], counts) and np.array_equal(z['nearest_row'], row) and z['nearest_dist'].shape == (n, nc)
    with pytest.raises(ValueError, match='neighbors needs measure=True'):
        evaluation.inference_on_slide(dep, slide, tile=256, overlap=32, batch_size=5, compute_masks=True, label_map=True, neighbors=(32,))
