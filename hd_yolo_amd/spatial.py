"""Neighbourhood features of a slide's nuclei: what relates one row of the nucleus table to another (ops.spatial_neighbors, ops.spatial_density:
csrc/spatial.hip, include/hdyolo_spatial.h).

The device passes work on integers: a position is int32 (x, y) in units of 1 / UNITS pixel (to_units: round(px * 16), so a centroid keeps four
binary places), a radius is int(round(r_px * 16)) units, "within r" is dx^2 + dy^2 <= r^2 in int64.  The counts and the nearest neighbours are
therefore a pure function of the table: no dependence on the search grid, the launch or the order of the rows.

    neighborhood(table_or_result, nc, radii_px)   per nucleus: neighbours of every class within every radius, the nearest of every class
    interaction_matrix(counts, cls, C)            per radius: ordered pairs (a, b) of classes that are neighbours, over the whole slide
    'density' (neighborhood(..., field_px=...))   per field of the slide: nuclei of every class

Everything is tensor arithmetic around the two device calls: no loop over rows, and nothing is read back when the slide's size is given.
"""
import torch

from . import _ext

UNITS = _ext.CONSTANTS['HDY_SPATIAL_SUBPIXEL']


def to_units(xy_px):
    """int32 positions in units of 1/16 pixel from positions in pixels (any float or integer dtype, any shape): round(px * 16) in float64, ties
    to even.  A position that is not finite becomes -1 (absent); so does one that passes the int32 range."""
    v = torch.round(xy_px.double() * UNITS)
    ok = torch.isfinite(v) & (v.abs() < 2.0 ** 31)
    return torch.where(ok, v, -1.0).to(torch.int32)


def radius_units(r_px):
    return int(round(float(r_px) * UNITS))


def _points(t, nc):
    """(xy int32 (N, 2) units, class int64 (N,)) of a nucleus table or a result"""
    if 'labels' not in t:
        raise ValueError("neighborhood: the table or result has no 'labels' (the class of a nucleus is labels - 1)")
    xy = _positions(t)
    cls = t['labels'].to(device=xy.device, dtype=torch.int64).reshape(-1) - 1
    return xy, torch.where((cls >= 0) & (cls < int(nc)), cls, -1)


def _positions(t):
    """xy int32 (N, 2) units of a nucleus table (centroids; rows of area 0 absent) or a result (box centres)"""
    if 'centroid_x' in t:
        xy = torch.stack([t['centroid_x'], t['centroid_y']], 1).double()
        if 'area' in t:
            xy = torch.where((t['area'] > 0)[:, None], xy, float('nan'))              # a row that owns nothing is absent
    elif 'boxes' in t:
        b = t['boxes'].reshape(-1, 4).double()
        xy = torch.stack([(b[:, 0] + b[:, 2]) * 0.5, (b[:, 1] + b[:, 3]) * 0.5], 1)
    else:
        raise ValueError("neighborhood: neither a nucleus table ('centroid_x', 'centroid_y') nor a result ('boxes')")
    return to_units(xy)


@torch.no_grad()
def neighborhood(table_or_result, nc, radii_px, field_px=None, size=None):
    """Neighbourhood columns of a nucleus table (measure.nucleus_table: positions = centroid_x / centroid_y, rows of area 0 absent) or of a
    result without one ('boxes': positions = box centres).  The class of a row is labels - 1; outside 0 .. nc - 1 the row is a query only: it gets
    its own columns and is counted by nobody.  radii_px: K strictly increasing radii in pixels of the table's coordinates.
      'neighbors'     int32 (N, K, nc)     other nuclei of class c within radius k (cumulative over the radii)
      'nearest_dist'  float64 (N, nc)      pixels to the nearest nucleus of class c within the largest radius, NaN where there is none
      'nearest_row'   int32 (N, nc)        its row, -1 where there is none
      'density'       int32 (gy, gx, nc)   with field_px: nuclei of class c per field_px x field_px field of the slide
    size = (H, W) of the slide in pixels: sizes the search grid and the fields without reading anything back; without it the largest
    coordinates are read once.  Absent rows (area 0, a position that is not finite or negative) hold 0, NaN and -1."""
    nc = int(nc)
    radii = [radius_units(r) for r in radii_px]
    xy, cls = _points(table_or_result, nc)
    N, K = xy.shape[0], len(radii)
    extent = None if size is None else (int(size[1]) * UNITS, int(size[0]) * UNITS)
    if N == 0:
        counts = torch.zeros((0, K, nc), dtype=torch.int32, device=xy.device)
        d2 = torch.zeros((0, nc), dtype=torch.int64, device=xy.device)
        row = torch.zeros((0, nc), dtype=torch.int32, device=xy.device)
    else:
        from . import ops
        counts, d2, row = ops.spatial_neighbors(xy, cls, nc, radii, extent_units=extent)
    out = {'neighbors': counts, 'nearest_dist': torch.where(d2 < 0, float('nan'), torch.sqrt(d2.double()) / UNITS), 'nearest_row': row}
    if field_px is not None:
        g = radius_units(field_px)
        if g < 1:
            raise ValueError(f'neighborhood: field_px={field_px} is less than a unit')
        if extent is None:
            extent = [int(v) + 1 for v in xy.amax(0).clamp(min=0).tolist()] if N else [1, 1]
        gx, gy = (max(-(-e // g), 1) for e in extent)
        if N == 0:
            out['density'] = torch.zeros((gy, gx, nc), dtype=torch.int32, device=xy.device)
        else:
            from . import ops
            out['density'] = ops.spatial_density(xy, cls, nc, g, gx, gy)
    return out


def interaction_matrix(counts, cls, C):
    """int64 (K, C, C): entry (k, a, b) = ordered pairs (p, q) with p of class a, q of class b and q within radius k of p, from neighborhood's
    'neighbors' (N, K, C) and the rows' classes (labels - 1; rows of a class outside [0, C) add nothing): one integer index_add_ on the device."""
    C = int(C)
    N, K = counts.shape[0], counts.shape[1]
    if counts.dim() != 3 or counts.shape[2] != C or tuple(cls.shape) != (N,):
        raise ValueError(f'interaction_matrix: counts {tuple(counts.shape)} and classes {tuple(cls.shape)} do not describe N rows of K x {C} counts')
    cls = cls.to(device=counts.device, dtype=torch.int64)
    index = torch.where((cls >= 0) & (cls < C), cls, C)                               # row C collects what no class owns
    acc = torch.zeros((C + 1, K, C), dtype=torch.int64, device=counts.device)
    acc.index_add_(0, index, counts.to(torch.int64))
    return acc[:C].permute(1, 0, 2).contiguous()
