"""Numpy restatement of the neighbourhood arithmetic of include/hdyolo_spatial.h (csrc/spatial.hip), by brute force over all pairs in int64,
and the point sets the host and GPU tests share.

    neighbors(xy, cls, C, radii)       -> counts int32 (N, K, C), near_d2 int64 (N, C), near_row int32 (N, C)      chunked (chunk x N) blocks
    neighbors_slow(xy, cls, C, radii)  the same by a plain Python double loop (small N)
    density(xy, cls, C, g, gx, gy)     -> grid int32 (gy, gx, C), by np.add.at

xy int (N, 2) units; a negative coordinate = absent; a class outside [0, C) = query only; a point is never its own neighbour (by row, not by
distance); within r: dx^2 + dy^2 <= r^2; nearest: smallest d2 within the largest radius, lowest row among equals, -1 / -1 for none.
"""
import numpy as np

UNITS = 16


def neighbors(xy, cls, C, radii, chunk=512):
    xy = np.asarray(xy, dtype=np.int64).reshape(-1, 2)
    cls = np.asarray(cls, dtype=np.int64).reshape(-1)
    N, K = len(xy), len(radii)
    r2 = [int(r) * int(r) for r in radii]
    present = (xy >= 0).all(1)
    counted = present & (cls >= 0) & (cls < C)
    counts = np.zeros((N, K, C), dtype=np.int32)
    near_d2 = np.full((N, C), -1, dtype=np.int64)
    near_row = np.full((N, C), -1, dtype=np.int32)
    rows = np.arange(N)
    big = np.iinfo(np.int64).max
    for q0 in range(0, N, chunk):
        q = slice(q0, min(q0 + chunk, N))
        dx = xy[q, None, 0] - xy[None, :, 0]
        dy = xy[q, None, 1] - xy[None, :, 1]
        d2 = dx * dx + dy * dy
        pair = present[q, None] & counted[None, :] & (rows[q, None] != rows[None, :])
        for c in range(C):
            m = pair & (cls == c)[None, :]
            for k in range(K):
                counts[q, k, c] = (m & (d2 <= r2[k])).sum(1)
            dm = np.where(m & (d2 <= r2[-1]), d2, big)
            arg = dm.argmin(1)                                   # the first of the minima: the lowest row
            best = dm[np.arange(dm.shape[0]), arg]
            hit = best < big
            near_d2[q, c] = np.where(hit, best, -1)
            near_row[q, c] = np.where(hit, arg, -1)
    return counts, near_d2, near_row


def neighbors_slow(xy, cls, C, radii):
    N, K = len(xy), len(radii)
    counts = np.zeros((N, K, C), dtype=np.int32)
    near_d2 = np.full((N, C), -1, dtype=np.int64)
    near_row = np.full((N, C), -1, dtype=np.int32)
    for p in range(N):
        px, py = int(xy[p][0]), int(xy[p][1])
        if px < 0 or py < 0:
            continue
        for q in range(N):
            qx, qy, c = int(xy[q][0]), int(xy[q][1]), int(cls[q])
            if q == p or qx < 0 or qy < 0 or not 0 <= c < C:
                continue
            d2 = (qx - px) ** 2 + (qy - py) ** 2
            for k in range(K):
                if d2 <= int(radii[k]) ** 2:
                    counts[p, k, c] += 1
            if d2 <= int(radii[-1]) ** 2 and (near_row[p, c] < 0 or d2 < near_d2[p, c]):       # q ascends: the first of equals stays
                near_d2[p, c], near_row[p, c] = d2, q
    return counts, near_d2, near_row


def density(xy, cls, C, g, gx, gy):
    xy = np.asarray(xy, dtype=np.int64).reshape(-1, 2)
    cls = np.asarray(cls, dtype=np.int64).reshape(-1)
    grid = np.zeros((gy, gx, C), dtype=np.int32)
    fx, fy = xy[:, 0] // g, xy[:, 1] // g
    ok = (xy >= 0).all(1) & (cls >= 0) & (cls < C) & (fx < gx) & (fy < gy)
    np.add.at(grid, (fy[ok], fx[ok], cls[ok]), 1)
    return grid


def interaction(counts, cls, C):
    """int64 (K, C, C): [k, a, b] = sum of counts[p, k, b] over the rows p of class a"""
    out = np.zeros((counts.shape[1], C, C), dtype=np.int64)
    for p in range(len(cls)):
        if 0 <= int(cls[p]) < C:
            out[:, int(cls[p]), :] += counts[p]
    return out


# ---- point sets ----------------------------------------------------------------------------------------------------------------------------
RADII = (16 * UNITS, 32 * UNITS, 64 * UNITS)          # 16 / 32 / 64 px


def uniform(rng, N, side_px=2048, C=3):
    return rng.integers(0, side_px * UNITS, (N, 2)).astype(np.int32), rng.integers(0, C, N).astype(np.int32)


def borders(cell, ncx=5, ncy=4, C=3):
    """points exactly on cell borders, at coordinate 0 and at the largest coordinate of an ncx x ncy grid of `cell` units, one unit to either
    side of every border, and pairs at exactly r = cell and r + 1 across borders: queries in every corner and edge cell"""
    xs = sorted({v for i in range(ncx + 1) for v in (i * cell - 1, i * cell, i * cell + 1) if 0 <= v < ncx * cell})
    ys = sorted({v for i in range(ncy + 1) for v in (i * cell - 1, i * cell, i * cell + 1) if 0 <= v < ncy * cell})
    xy = np.array([(x, y) for y in ys for x in xs], dtype=np.int32)
    cls = (np.arange(len(xy)) % C).astype(np.int32)
    return xy, cls


def lattice(n=24, step=8 * UNITS, C=3):
    """an integer lattice: many equal distances, so the tie rule decides most nearest rows"""
    yy, xx = np.meshgrid(np.arange(n), np.arange(n), indexing='ij')
    xy = np.stack([xx.ravel() * step, yy.ravel() * step], 1).astype(np.int32)
    return xy, ((xx.ravel() + 2 * yy.ravel()) % C).astype(np.int32)


def mixed(rng, N=700, side_px=512, C=3):
    """uniform points with query-only classes (-1, C, 2^31 - 1) and absent points (either coordinate negative) mixed in"""
    xy, cls = uniform(rng, N, side_px, C)
    kind = rng.integers(0, 8, N)
    cls[kind == 0] = -1
    cls[kind == 1] = C
    cls[kind == 2] = 2 ** 31 - 1
    xy[kind == 3, 0] = -1
    xy[kind == 4, 1] = -(2 ** 31)
    xy[(kind == 5) & (np.arange(N) % 2 == 0)] = -7
    return xy, cls
