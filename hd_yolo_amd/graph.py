"""The cell graph of a slide's nuclei: every nucleus joined to its k nearest neighbours (ops.spatial_knn, ops.knn_mutual: csrc/graph.hip,
include/hdyolo_graph.h).

Positions and distances are those of hd_yolo_amd/spatial.py: int32 units of 1/16 pixel, squared distances in int64, so the neighbours, their
order and the edge list are a pure function of the table: no dependence on the search grid, the launch or the order of the rows.

    knn_graph(table_or_result, k, max_px)     per nucleus: the rows of its k nearest nuclei within max_px, their distances, which are mutual
    edges(graph, mode)                        the edge list: 'union' / 'mutual' (undirected, p < q) or 'directed'
    node_features(graph, cls, nc)             per nucleus: mean / min / max neighbour distance, in-degree, neighbours of every class
    save_cell_graph(path, graph, edges)       .npz, one device-to-host copy

Everything is tensor arithmetic around the two device calls, with no loop over rows; edges, node_features and save_cell_graph take CPU tensors
too.
"""
import numpy as np
import torch

from .spatial import UNITS, _points, _positions, radius_units

GRAPH_KEYS = ('knn_row', 'knn_dist', 'knn_count', 'knn_mutual')
EDGE_KEYS = ('edge_index', 'edge_dist', 'edge_mutual')


@torch.no_grad()
def knn_graph(table_or_result, k, max_px, nc=None, size=None):
    """The k nearest neighbours of every row of a nucleus table (measure.nucleus_table: positions = centroid_x / centroid_y, rows of area 0
    absent) or of a result without one ('boxes': positions = box centres).  With nc the class of a row is labels - 1 and a row of a class
    outside 0 .. nc - 1 is a query only: it gets neighbours and is nobody's; without nc every present row is a node.  A neighbour lies within
    max_px pixels of the table's coordinates; 1 <= k <= 16.
      'knn_row'     int32 (N, k)      the rows of the neighbours, nearest first, equal distances by the lowest row; -1 padding
      'knn_dist'    float64 (N, k)    pixels, sqrt(d2) / 16; NaN padding
      'knn_count'   int32 (N,)        how many neighbours the row has
      'knn_mutual'  bool (N, k)       the neighbour has this row among its own k
    size = (H, W) of the slide in pixels: sizes the search grid without reading anything back; without it the largest coordinates are read
    once.  Absent rows (area 0, a position that is not finite or negative) hold -1, NaN, 0 and False."""
    k, r = int(k), radius_units(max_px)
    if nc is None:
        xy, cls = _positions(table_or_result), None
    else:
        xy, cls = _points(table_or_result, int(nc))
    N = xy.shape[0]
    extent = None if size is None else (int(size[1]) * UNITS, int(size[0]) * UNITS)
    if N == 0:
        from . import _ext
        max_k = _ext.CONSTANTS['HDY_GRAPH_MAX_K']
        if not 1 <= k <= max_k:
            raise ValueError(f'knn_graph: k={k} outside [1, {max_k}]')
        row = torch.zeros((0, k), dtype=torch.int32, device=xy.device)
        d2 = torch.zeros((0, k), dtype=torch.int64, device=xy.device)
        count = torch.zeros((0,), dtype=torch.int32, device=xy.device)
        mutual = torch.zeros((0, k), dtype=torch.int32, device=xy.device)
    else:
        from . import ops
        row, d2, count = ops.spatial_knn(xy, k, r, cls=cls, C=None if nc is None else int(nc), extent_units=extent)
        mutual = ops.knn_mutual(row)
    return {'knn_row': row, 'knn_dist': torch.where(d2 < 0, float('nan'), torch.sqrt(d2.double()) / UNITS), 'knn_count': count,
            'knn_mutual': mutual != 0}


def _directed(graph):
    row = graph['knn_row']
    N = row.shape[0]
    held = row >= 0
    p = torch.arange(N, dtype=torch.int64, device=row.device)[:, None].expand_as(row)[held]
    return N, p, row[held].to(torch.int64), graph['knn_dist'][held], graph['knn_mutual'][held]


@torch.no_grad()
def edges(graph, mode='union'):
    """The edge list of a knn_graph.
      'directed'   every (p, q = knn_row[p, s]), in (p, s) order; 'edge_mutual': (q, p) is an edge too
      'union'      the pairs {p, q} joined in either direction, each once as p < q, sorted by (p, q); 'edge_mutual': joined in both
      'mutual'     of those, the pairs joined in both directions
    'edge_index' int64 (2, E), 'edge_dist' float64 (E,) pixels, 'edge_mutual' bool (E,).  The number of edges is the one scalar read back."""
    if mode not in ('union', 'mutual', 'directed'):
        raise ValueError(f"edges: mode {mode!r} is none of 'union', 'mutual', 'directed'")
    N, p, q, dist, both = _directed(graph)
    if mode == 'directed':
        return {'edge_index': torch.stack([p, q]), 'edge_dist': dist, 'edge_mutual': both}
    lo, hi = torch.minimum(p, q), torch.maximum(p, q)
    key, inverse = torch.unique(lo * max(N, 1) + hi, return_inverse=True)       # sorted; a mutual pair occurs twice, with one distance
    edge_dist = torch.empty(key.shape, dtype=dist.dtype, device=dist.device)
    edge_both = torch.empty(key.shape, dtype=torch.bool, device=dist.device)
    edge_dist[inverse] = dist                                                    # both copies of a pair write the same values
    edge_both[inverse] = both
    index = torch.stack([torch.div(key, max(N, 1), rounding_mode='floor'), key % max(N, 1)])
    if mode == 'mutual':
        index, edge_dist, edge_both = index[:, edge_both], edge_dist[edge_both], edge_both[edge_both]
    return {'edge_index': index, 'edge_dist': edge_dist, 'edge_mutual': edge_both}


@torch.no_grad()
def node_features(graph, cls=None, nc=None):
    """Per row of a knn_graph:
      'knn_mean_dist', 'knn_min_dist', 'knn_max_dist'   float64 (N,)   over the row's neighbours, NaN for a row without any; the mean is the
                                                                       sum over the slots in order, divided by the count
      'in_degree'                                       int32 (N,)     how many rows have this one among their neighbours
      'knn_class_counts' (with cls and nc)              int32 (N, nc)  the row's neighbours of every class; cls (N,) = labels - 1, a neighbour
                                                                       of a class outside 0 .. nc - 1 is counted nowhere"""
    row, dist, count = graph['knn_row'], graph['knn_dist'], graph['knn_count']
    N, k = row.shape
    held = row >= 0
    total = torch.zeros((N,), dtype=torch.float64, device=row.device)
    for s in range(k):                                                           # slots, not rows: a fixed order of additions
        total = total + torch.where(held[:, s], dist[:, s], 0.0)
    none = count <= 0
    nan = torch.full((N,), float('nan'), dtype=torch.float64, device=row.device)
    last = (count.to(torch.int64) - 1).clamp(min=0)[:, None]
    out = {'knn_mean_dist': torch.where(none, nan, total / count.clamp(min=1).double()),
           'knn_min_dist': torch.where(none, nan, dist[:, 0]) if k else nan,
           'knn_max_dist': torch.where(none, nan, dist.gather(1, last)[:, 0]) if k else nan,
           'in_degree': torch.bincount(row[held].to(torch.int64), minlength=N)[:N].to(torch.int32)}
    if (cls is None) != (nc is None):
        raise ValueError('node_features: cls and nc go together')
    if cls is not None:
        nc = int(nc)
        cls = cls.to(device=row.device, dtype=torch.int64).reshape(-1)
        if cls.shape[0] != N:
            raise ValueError(f'node_features: {cls.shape[0]} classes for {N} rows')
        p = torch.arange(N, dtype=torch.int64, device=row.device)[:, None].expand_as(row)[held]
        c = cls[row[held].to(torch.int64)]
        ok = (c >= 0) & (c < nc)
        out['knn_class_counts'] = torch.bincount(p[ok] * nc + c[ok], minlength=N * nc)[:N * nc].reshape(N, nc).to(torch.int32)
    return out


def save_cell_graph(path, graph, edges, xy=None, labels=None):
    """Write a knn_graph and its edge list to `path` (.npz): 'edge_index', 'edge_dist', 'edge_mutual', 'knn_row', 'knn_dist', 'knn_count',
    'knn_mutual' and, when given, 'xy' (N, 2) positions and 'labels' (N,).  The arrays are packed into one byte buffer on their device, so the
    file costs one device-to-host copy."""
    if not str(path).endswith('.npz'):
        raise ValueError(f'save_cell_graph: {path!r} is not an .npz path')
    arrays = {k: edges[k] for k in EDGE_KEYS}
    arrays.update({k: graph[k] for k in GRAPH_KEYS})
    if xy is not None:
        arrays['xy'] = xy
    if labels is not None:
        arrays['labels'] = labels
    dev = arrays['knn_row'].device
    parts = []
    for name, t in arrays.items():
        t = t.detach().to(dev).contiguous()
        parts.append((name, t.dtype, tuple(t.shape), (t.to(torch.uint8) if t.dtype == torch.bool else t).reshape(-1).view(torch.uint8)))
    host = (torch.cat([b for *_, b in parts]) if parts else torch.zeros(0, dtype=torch.uint8)).cpu()
    out, at = {}, 0
    for name, dtype, shape, b in parts:
        piece = host[at:at + b.numel()].clone()
        at += b.numel()
        out[name] = (piece.bool() if dtype == torch.bool else piece.view(dtype)).reshape(shape).numpy()
    np.savez(path, **out)
