"""numpy restatement of hdy_label_measure (include/hdyolo_measure.h), twice: `measure` vectorised with np.add.at in int64 (numpy's int64 adds and
products wrap modulo 2^64 as the contract demands), `measure_slow` as a loop over labels on boolean masks with Python integers reduced modulo
2^64 at the end.  Plus `table`, the float64 restatement of hd_yolo_amd/measure.py's formulas from the same sums, and a few map makers."""
import numpy as np

COLS = 14
MASK64 = (1 << 64) - 1


def _different(lm):
    """per entry: (number of the four neighbours outside the window or of another raw value, number of them outside the window)"""
    h, w = lm.shape
    pad = np.full((h + 2, w + 2), np.int64(1) << 40, dtype=np.int64)         # no int32 value: 'outside' differs from everything
    pad[1:-1, 1:-1] = lm
    c = pad[1:-1, 1:-1]
    edges = (pad[:-2, 1:-1] != c).astype(np.int64) + (pad[2:, 1:-1] != c) + (pad[1:-1, :-2] != c) + (pad[1:-1, 2:] != c)
    ii, jj = np.mgrid[0:h, 0:w]
    border = (ii == 0).astype(np.int64) + (ii == h - 1) + (jj == 0) + (jj == w - 1)
    return edges, border


def measure(lm, R, image=None, window=(0, 0), origin=None):
    """(sums int64 (R, 14), extent int32 (R, 4)); image: uint8 (H, W, 3 | 4) of which the map covers the window at (x0, y0) = window"""
    lm = np.asarray(lm, dtype=np.int32)
    h, w = lm.shape
    sums = np.zeros((R, COLS), dtype=np.int64)
    extent = np.tile(np.array([w, h, -1, -1], dtype=np.int32), (R, 1))
    own = (lm >= 0) & (lm < R)
    ii, jj = np.nonzero(own)
    r = lm[ii, jj].astype(np.int64)
    org = np.zeros((R, 2), dtype=np.int64) if origin is None else np.asarray(origin, dtype=np.int64).reshape(R, 2)
    with np.errstate(over='ignore'):
        dx, dy = jj.astype(np.int64) - org[r, 0], ii.astype(np.int64) - org[r, 1]
        edges, border = _different(lm)
        cols = [np.ones_like(dx), dx, dy, dx * dx, dy * dy, dx * dy, edges[ii, jj], border[ii, jj]]
        if image is not None:
            x0, y0 = window
            px = np.asarray(image)[y0 + ii, x0 + jj, :3].astype(np.int64)
            cols += [px[:, 0], px[:, 1], px[:, 2], px[:, 0] ** 2, px[:, 1] ** 2, px[:, 2] ** 2]
        for c, v in enumerate(cols):
            np.add.at(sums[:, c], r, v)
    np.minimum.at(extent[:, 0], r, jj.astype(np.int32))
    np.minimum.at(extent[:, 1], r, ii.astype(np.int32))
    np.maximum.at(extent[:, 2], r, jj.astype(np.int32))
    np.maximum.at(extent[:, 3], r, ii.astype(np.int32))
    return sums, extent


def _wrap(v):
    v &= MASK64
    return v - (1 << 64) if v >> 63 else v


def measure_slow(lm, R, image=None, window=(0, 0), origin=None):
    """the same, one label at a time on boolean masks, in Python integers"""
    lm = np.asarray(lm, dtype=np.int32)
    h, w = lm.shape
    sums = np.zeros((R, COLS), dtype=np.int64)
    extent = np.tile(np.array([w, h, -1, -1], dtype=np.int32), (R, 1))
    for r in range(R):
        mask = lm == r
        if not mask.any():
            continue
        ox, oy = (0, 0) if origin is None else (int(origin[r][0]), int(origin[r][1]))
        row = [0] * COLS
        for i, j in zip(*np.nonzero(mask)):
            i, j = int(i), int(j)
            dx, dy = j - ox, i - oy
            row[0] += 1
            row[1] += dx
            row[2] += dy
            row[3] += dx * dx
            row[4] += dy * dy
            row[5] += dx * dy
            for ni, nj in ((i - 1, j), (i + 1, j), (i, j - 1), (i, j + 1)):
                outside = ni < 0 or ni >= h or nj < 0 or nj >= w
                if outside or lm[ni, nj] != r:
                    row[6] += 1
                row[7] += int(outside)
            if image is not None:
                p = image[window[1] + i, window[0] + j]
                for c in range(3):
                    row[8 + c] += int(p[c])
                    row[11 + c] += int(p[c]) ** 2
        sums[r] = [_wrap(v) for v in row]
        ys, xs = np.nonzero(mask)
        extent[r] = [xs.min(), ys.min(), xs.max(), ys.max()]
    return sums, extent


def table(sums, extent, origin=None, offset=(0, 0)):
    """hd_yolo_amd/measure.py's formulas in numpy float64 from the same sums (module docstring there)"""
    sums = np.asarray(sums, dtype=np.int64)
    R = len(sums)
    n, sx, sy, sxx, syy, sxy, edges, border = (sums[:, c] for c in range(8))
    org = np.zeros((R, 2), dtype=np.int64) if origin is None else np.asarray(origin, dtype=np.int64)
    nf = n.astype(np.float64)
    t = {'area': n, 'perimeter_edges': edges, 'border_edges': border, 'touches_border': border > 0}
    with np.errstate(all='ignore'):
        t['centroid_x'] = org[:, 0].astype(np.float64) + sx.astype(np.float64) / nf + float(offset[0])
        t['centroid_y'] = org[:, 1].astype(np.float64) + sy.astype(np.float64) / nf + float(offset[1])
        ext = np.asarray(extent, dtype=np.int64)
        t['bbox'] = np.where((n > 0)[:, None], ext + np.array([offset[0], offset[1]] * 2, dtype=np.int64), ext)
        n2 = nf * nf
        mu20, mu02, mu11 = (n * sxx - sx * sx) / n2, (n * syy - sy * sy) / n2, (n * sxy - sx * sy) / n2
        half, diff = (mu20 + mu02) / 2, (mu20 - mu02) / 2
        root = np.sqrt(diff * diff + mu11 * mu11)
        lp, lm = half + root, half - root
        t['lambda_plus'], t['lambda_minus'] = lp, lm
        t['major_axis'] = 4 * np.sqrt(lp)
        t['minor_axis'] = 4 * np.sqrt(np.maximum(lm, 0))
        t['eccentricity'] = np.where(lp == 0, 0.0, np.sqrt(1 - lm / lp))
        t['orientation'] = np.arctan2(2 * mu11, mu20 - mu02) / 2
        t['equivalent_diameter'] = np.sqrt(4 * nf / np.pi)
        ef = edges.astype(np.float64)
        t['compactness'] = 16 * nf / (ef * ef)
        sc, scc = sums[:, 8:11], sums[:, 11:14]
        t['mean_rgb'] = sc / nf[:, None]
        t['std_rgb'] = np.sqrt(np.maximum(n[:, None] * scc - sc * sc, 0).astype(np.float64)) / nf[:, None]
    return t


INT_COLUMNS = ('area', 'perimeter_edges', 'border_edges', 'touches_border', 'bbox')
FLOAT_COLUMNS = ('centroid_x', 'centroid_y', 'major_axis', 'minor_axis', 'equivalent_diameter', 'compactness', 'mean_rgb', 'std_rgb')


def assert_tables_agree(got, want):
    """`got`: nucleus_table's columns as numpy arrays; `want`: table() from the same sums.  Integer columns equal; float columns rtol 1e-12 (each
    at most about ten correctly rounded float64 operations on exact integers); eccentricity and orientation atol 1e-7 (the square root and the
    angle amplify a 1e-16 error when lambda+ ~ lambda-), orientation only where lambda+ >= 1.5 lambda-.  NaN rows (n = 0) must be NaN on both sides."""
    for k in INT_COLUMNS:
        assert np.array_equal(np.asarray(got[k]), want[k]), k
    for k in FLOAT_COLUMNS:
        if k in got:
            np.testing.assert_allclose(np.asarray(got[k]), want[k], rtol=1e-12, atol=0, equal_nan=True, err_msg=k)
    np.testing.assert_allclose(np.asarray(got['eccentricity']), want['eccentricity'], rtol=0, atol=1e-7, equal_nan=True)
    sel = want['lambda_plus'] >= 1.5 * want['lambda_minus']
    np.testing.assert_allclose(np.asarray(got['orientation'])[sel], want['orientation'][sel], rtol=0, atol=1e-7, equal_nan=True)


def random_map(rng, h, w, R, labels_above=3):
    """blobs of labels in [0, R + labels_above) on a background of assorted non-labels"""
    lm = rng.choice(np.array([-1, -7, 0x7fffffff, R], dtype=np.int64), size=(h, w)).astype(np.int32)
    for _ in range(max(1, (h * w) // 40)):
        r = int(rng.integers(0, R + labels_above))
        i, j = int(rng.integers(0, h)), int(rng.integers(0, w))
        a, b = int(rng.integers(1, 9)), int(rng.integers(1, 9))
        lm[i:i + a, j:j + b] = r
    return lm
