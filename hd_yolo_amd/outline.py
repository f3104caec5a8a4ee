"""Shape columns and polygon files from the outlines and hulls of ops.label_outline / ops.label_hull (csrc/outline.hip,
include/hdyolo_outline.h).

shape_table is tensor arithmetic on whole columns, on whatever device its inputs live, with no loop over rows and no read of a value.  With n
and E the columns 0 and 6 of ops.label_measure's sums, counts = {V, twice the enclosed area, cracks L, flags} and hull_i = {H, twice the hull
area A2, squared maximum Feret diameter F2, flags}, hull_f = {hull perimeter P, minimum Feret diameter}:

    outline_vertices   V
    outline_edges      L: the unit pixel edges of the outline
    enclosed_area      pixels inside the outline: the label's first component and its holes
    simple             enclosed_area == n and L == E: one 4-connected component without a hole, and nothing else of the label elsewhere
    convex_area        A2 / 2
    solidity           2 n / A2
    convex_perimeter   P
    convexity          P / L
    feret_max          sqrt(F2)
    feret_min          the smallest caliper width
    feret_ratio        feret_min / feret_max

Every float column is NaN, and simple is False, where n = 0 or the label was flagged by either pass (an empty extent, a box side above
HDY_OUTLINE_MAX_SIDE, an extent that was not the map's); the integer columns of such a row are zero.

save_polygons / load_polygons: the outlines as the CSR arrays (.npz) or as a GeoJSON FeatureCollection (.geojson), one closed ring per nucleus.
"""
import json
import os

import torch

SHAPE_COLUMNS = ('outline_vertices', 'outline_edges', 'enclosed_area', 'simple', 'convex_area', 'solidity', 'convex_perimeter', 'convexity',
                 'feret_max', 'feret_min', 'feret_ratio')


def shape_table(sums, counts, hull_i, hull_f):
    """dict of per-label shape columns (see the module docstring) from ops.label_measure's sums, ops.label_outline's counts and ops.label_hull's
    (hull_i, hull_f)."""
    if sums.dtype != torch.int64 or sums.dim() != 2 or sums.shape[1] < 7:
        raise ValueError(f'shape_table: sums must be int64 (R, 14), got {sums.dtype} {tuple(sums.shape)}')
    R = sums.shape[0]
    for name, t, dt, cols in (('counts', counts, torch.int64, 4), ('hull_i', hull_i, torch.int64, 4), ('hull_f', hull_f, torch.float64, 2)):
        if t.dtype != dt or tuple(t.shape) != (R, cols):
            raise ValueError(f'shape_table: {name} must be {dt} ({R}, {cols}), got {t.dtype} {tuple(t.shape)}')
    f64 = torch.float64
    nan = torch.full((R,), float('nan'), dtype=f64, device=sums.device)
    n, edges = sums[:, 0], sums[:, 6]
    V, area2, L = counts[:, 0], counts[:, 1], counts[:, 2]
    ok = (n > 0) & (counts[:, 3] == 0) & (hull_i[:, 3] == 0)
    enclosed = area2 // 2                                                  # area2 is even: twice a number of pixels
    hull_area2 = hull_i[:, 1].to(f64)

    def where_ok(v):
        return torch.where(ok, v, nan)

    fmax = torch.sqrt(hull_i[:, 2].to(f64))
    table = {'outline_vertices': V, 'outline_edges': L, 'enclosed_area': enclosed, 'simple': ok & (enclosed == n) & (L == edges)}
    table['convex_area'] = where_ok(hull_area2 / 2)
    table['solidity'] = where_ok(2 * n.to(f64) / hull_area2)
    table['convex_perimeter'] = where_ok(hull_f[:, 0])
    table['convexity'] = where_ok(hull_f[:, 0] / L.to(f64))
    table['feret_max'] = where_ok(fmax)
    table['feret_min'] = where_ok(hull_f[:, 1])
    table['feret_ratio'] = where_ok(hull_f[:, 1] / fmax)
    return table


def _host(t, dtype):
    import numpy as np
    return np.ascontiguousarray((t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).astype(dtype, copy=False))


def save_polygons(path, offsets, verts, offset=(0, 0), scale=1.0, labels=None, scores=None):
    """Write the outlines of ops.label_outline by the extension of `path`.
    .npz: the CSR arrays as they are ('offsets' int64 (R + 1,), 'verts' int32 (total, 2)) with 'offset', 'scale' and, when given, 'labels' /
    'scores'.
    .geojson: a FeatureCollection with one Feature per nucleus with V > 0, its geometry a Polygon of one closed ring (the first vertex again at
    the end) of coordinates (vertex + offset) / scale, its properties {'row', 'classification' (labels), 'score' (scores)}.
    offset = (x, y) of the map's window in the slide, scale = the magnification the map was drawn at, so that coordinates are the slide's."""
    import numpy as np
    ext = os.path.splitext(path)[1].lower()
    if ext not in ('.npz', '.geojson'):
        raise ValueError(f'save_polygons: {path!r} is neither .npz nor .geojson')
    off, vs = _host(offsets, np.int64), _host(verts, np.int32).reshape(-1, 2)
    R = len(off) - 1
    if R < 0 or (R >= 0 and len(off) and (int(off[0]) != 0 or int(off[-1]) != len(vs) or (np.diff(off) < 0).any())):
        raise ValueError(f'save_polygons: offsets do not describe the {len(vs)} rows of verts')
    lab = None if labels is None else _host(labels, np.int64)
    sco = None if scores is None else _host(scores, np.float64)
    if ext == '.npz':
        extra = {k: v for k, v in (('labels', lab), ('scores', sco)) if v is not None}
        np.savez(path, offsets=off, verts=vs, offset=np.asarray([float(offset[0]), float(offset[1])]), scale=np.asarray(float(scale)), **extra)
        return
    xy = (vs.astype(np.float64) + np.asarray([float(offset[0]), float(offset[1])])) / float(scale)
    features = []
    for r in range(R):
        a, b = int(off[r]), int(off[r + 1])
        if b == a:
            continue
        ring = xy[a:b].tolist()
        ring.append(ring[0])
        props = {'row': r}
        if lab is not None:
            props['classification'] = int(lab[r])
        if sco is not None:
            props['score'] = float(sco[r])
        features.append({'type': 'Feature', 'geometry': {'type': 'Polygon', 'coordinates': [ring]}, 'properties': props})
    with open(path, 'w') as f:
        json.dump({'type': 'FeatureCollection', 'features': features}, f)


def load_polygons(path):
    """What save_polygons wrote, as a dict of numpy arrays.  .npz: its arrays.  .geojson: 'rows' int64 (P,), 'offsets' int64 (P + 1,) and
    'verts' float64 (total, 2) of the P rings without their closing vertex, and 'labels' / 'scores' when the file carries them."""
    import numpy as np
    if os.path.splitext(path)[1].lower() == '.npz':
        with np.load(path) as z:
            return {k: z[k] for k in z.files}
    with open(path) as f:
        doc = json.load(f)
    rows, offsets, verts, labels, scores = [], [0], [], [], []
    for feat in doc['features']:
        ring = feat['geometry']['coordinates'][0][:-1]
        verts.extend(ring)
        offsets.append(len(verts))
        props = feat['properties']
        rows.append(props['row'])
        if 'classification' in props:
            labels.append(props['classification'])
        if 'score' in props:
            scores.append(props['score'])
    out = {'rows': np.asarray(rows, dtype=np.int64), 'offsets': np.asarray(offsets, dtype=np.int64),
           'verts': np.asarray(verts, dtype=np.float64).reshape(-1, 2)}
    if labels:
        out['labels'] = np.asarray(labels, dtype=np.int64)
    if scores:
        out['scores'] = np.asarray(scores, dtype=np.float64)
    return out
