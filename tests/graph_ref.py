"""Numpy restatement of the k-nearest-neighbour arithmetic of include/hdyolo_graph.h (csrc/graph.hip), and of the edge lists of
hd_yolo_amd/graph.py.  The point sets are those of spatial_ref (uniform, borders, lattice, mixed).

    knn(xy, cls, k, r)                           -> nbr_row int32 (N, k), nbr_d2 int64 (N, k), nbr_count int32 (N,)   brute force, chunked
    knn_slow(xy, cls, k, r)                      the same by a plain Python double loop and sorted() (small N)
    mutual(nbr_row)                              -> int32 (N, k)
    ring_search(xy, cls, k, r, cell, ncx, ncy)   the same answer as knn by the kernel's traversal: rings of cells and the stop rule
    edges(nbr_row, nbr_d2, mode)                 -> edge_index int64 (2, E), edge_d2 int64 (E,), edge_mutual bool (E,)

xy int (N, 2) units; a negative coordinate = absent; cls None = every present point is a node, else a negative class = query only; a point is
never its own neighbour (by row, not by distance); candidates: dx^2 + dy^2 <= r^2; neighbours: the first k in (d2, row) order; -1 padding.
"""
import numpy as np

from spatial_ref import UNITS, borders, lattice, mixed, uniform  # noqa: F401  (the shared point sets)


def _inputs(xy, cls):
    xy = np.asarray(xy, dtype=np.int64).reshape(-1, 2)
    cls = np.zeros(len(xy), dtype=np.int64) if cls is None else np.asarray(cls, dtype=np.int64).reshape(-1)
    present = (xy >= 0).all(1)
    return xy, present, present & (cls >= 0)


def knn(xy, cls, k, r, chunk=512):
    xy, present, node = _inputs(xy, cls)
    N, r2 = len(xy), int(r) * int(r)
    nbr_row = np.full((N, k), -1, dtype=np.int32)
    nbr_d2 = np.full((N, k), -1, dtype=np.int64)
    nbr_count = np.zeros(N, dtype=np.int32)
    rows = np.arange(N)
    big = np.iinfo(np.int64).max
    for q0 in range(0, N, chunk):
        q = slice(q0, min(q0 + chunk, N))
        dx = xy[q, None, 0] - xy[None, :, 0]
        dy = xy[q, None, 1] - xy[None, :, 1]
        d2 = dx * dx + dy * dy
        ok = present[q, None] & node[None, :] & (rows[q, None] != rows[None, :]) & (d2 <= r2)
        key = np.where(ok, d2, big)
        for i in range(key.shape[0]):
            order = np.lexsort((rows, key[i]))[:k]                # ascending d2, then row
            order = order[key[i][order] < big]
            n = len(order)
            nbr_row[q0 + i, :n], nbr_d2[q0 + i, :n], nbr_count[q0 + i] = order, key[i][order], n
    return nbr_row, nbr_d2, nbr_count


def knn_slow(xy, cls, k, r):
    N = len(xy)
    nbr_row = np.full((N, k), -1, dtype=np.int32)
    nbr_d2 = np.full((N, k), -1, dtype=np.int64)
    nbr_count = np.zeros(N, dtype=np.int32)
    for p in range(N):
        px, py = int(xy[p][0]), int(xy[p][1])
        if px < 0 or py < 0:
            continue
        cand = []
        for q in range(N):
            qx, qy = int(xy[q][0]), int(xy[q][1])
            if q == p or qx < 0 or qy < 0 or (cls is not None and int(cls[q]) < 0):
                continue
            d2 = (qx - px) ** 2 + (qy - py) ** 2
            if d2 <= int(r) ** 2:
                cand.append((d2, q))
        for s, (d2, q) in enumerate(sorted(cand)[:k]):
            nbr_row[p, s], nbr_d2[p, s] = q, d2
        nbr_count[p] = min(len(cand), k)
    return nbr_row, nbr_d2, nbr_count


def mutual(nbr_row):
    nbr_row = np.asarray(nbr_row)
    N, k = nbr_row.shape
    out = np.zeros((N, k), dtype=np.int32)
    for p in range(N):
        for s in range(k):
            q = int(nbr_row[p, s])
            if 0 <= q < N and p in nbr_row[q].tolist():
                out[p, s] = 1
    return out


def ring_search(xy, cls, k, r, cell, ncx, ncy, stats=None):
    """The kernel's search, lane by lane: points binned by the cell rule (a coordinate beyond the grid in the last column / row), ring t = the
    cells at Chebyshev distance t, the stop rule after every ring.  The list of a lane is kept as a sorted Python list cut to k.  stats (a dict)
    receives 'last_ring', the ring after which every row stopped (-1 for absent rows)."""
    xy, present, node = _inputs(xy, cls)
    N = len(xy)
    r, cell = int(r), int(cell)
    rings = -(-r // cell)
    cells = {}
    for q in range(N):
        if present[q]:
            cells.setdefault((min(int(xy[q, 0]) // cell, ncx - 1), min(int(xy[q, 1]) // cell, ncy - 1)), []).append(q)
    nbr_row = np.full((N, k), -1, dtype=np.int32)
    nbr_d2 = np.full((N, k), -1, dtype=np.int64)
    nbr_count = np.zeros(N, dtype=np.int32)
    last = np.full(N, -1, dtype=np.int64)
    for p in range(N):
        if not present[p]:
            continue
        px, py = int(xy[p, 0]), int(xy[p, 1])
        cx, cy = min(px // cell, ncx - 1), min(py // cell, ncy - 1)
        best = []
        for t in range(rings + 1):
            ring = [(ix, iy) for iy in range(max(cy - t, 0), min(cy + t, ncy - 1) + 1) for ix in range(max(cx - t, 0), min(cx + t, ncx - 1) + 1)
                    if max(abs(ix - cx), abs(iy - cy)) == t]
            for c in ring:
                for q in cells.get(c, ()):
                    d2 = (int(xy[q, 0]) - px) ** 2 + (int(xy[q, 1]) - py) ** 2
                    if q != p and node[q] and d2 <= r * r:
                        best.append((d2, q))
            best = sorted(best)[:k]
            last[p] = t
            reach = t * cell
            if reach >= r:
                break
            if len(best) == k and best[-1][0] <= reach * reach:
                break
            if cx - t <= 0 and cx + t >= ncx - 1 and cy - t <= 0 and cy + t >= ncy - 1:
                break
        for s, (d2, q) in enumerate(best):
            nbr_row[p, s], nbr_d2[p, s] = q, d2
        nbr_count[p] = len(best)
    if stats is not None:
        stats['last_ring'] = last
    return nbr_row, nbr_d2, nbr_count


def dist(nbr_d2):
    """float64 pixels of squared units, NaN for the -1 padding"""
    d2 = np.asarray(nbr_d2)
    return np.where(d2 < 0, np.nan, np.sqrt(np.maximum(d2, 0).astype(np.float64)) / UNITS)


def edges(nbr_row, nbr_d2, mode='union'):
    """directed: every (p, q = nbr_row[p][s]) in (p, s) order.  union / mutual: the unordered pairs {p, q} that occur in either / in both
    directions, as p < q sorted by (p, q).  edge_mutual: whether the reverse (or for an undirected pair: both) direction occurs."""
    nbr_row = np.asarray(nbr_row)
    directed = {}
    for p in range(nbr_row.shape[0]):
        for s in range(nbr_row.shape[1]):
            if nbr_row[p, s] >= 0:
                directed[(p, int(nbr_row[p, s]))] = int(nbr_d2[p, s])
    if mode == 'directed':
        keys = list(directed)
        both = [(q, p) in directed for p, q in keys]
    else:
        pairs = {}
        for (p, q), d2 in directed.items():
            pairs[(min(p, q), max(p, q))] = d2
        keys = sorted(pairs)
        both = [(p, q) in directed and (q, p) in directed for p, q in keys]
        if mode == 'mutual':
            keys = [e for e, b in zip(keys, both) if b]
            both = [True] * len(keys)
        elif mode != 'union':
            raise ValueError(mode)
        directed = pairs
    index = np.array(keys, dtype=np.int64).reshape(-1, 2).T
    return index, np.array([directed[e] for e in keys], dtype=np.int64), np.array(both, dtype=bool)
