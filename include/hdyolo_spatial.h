/* hdyolo_spatial.h — extension header of libhdyolo_hip.so: neighbourhood features of a slide's nuclei (csrc/spatial.hip).
 *
 * An extension header declares entry points that are not part of the numbered ABI of hdyolo.h: it carries a revision of its own
 * (HDY_SPATIAL_REVISION, hdy_spatial_revision()), is bound by hd_yolo_amd/_ext.py and leaves HDY_ABI_VERSION alone.  The conventions are
 * hdyolo.h's: plain pointers and sizes, caller-owned buffers, everything on `stream`, 0 = ok, < 0 = invalid argument (hdy_last_error() says
 * which), > 0 = a hipError_t.
 *
 * ---- a binned neighbour search over the rows of a nucleus table ---------------------------------------------------------------------------
 * The three passes relate one nucleus to another: how many nuclei of every class lie within each of K radii of every nucleus, which one of
 * every class is the nearest, and how many nuclei of every class fall into every field of a coarse grid.  The reference has no counterpart
 * (it relates no detection to another); the arithmetic below is this project's own, all of it integer, restated in tests/spatial_ref.py.
 *
 * points.  pts int32 [N][4] = (x, y, class, original row), pts_elems = 4 * N exactly, 16-byte aligned (one 16-byte load per point).  x, y are
 * positions in units of 1 / HDY_SPATIAL_SUBPIXEL pixel; valid coordinates satisfy 0 <= x, y < HDY_SPATIAL_MAX_COORD.  A point with a negative
 * coordinate is ABSENT: it is nobody's neighbour, it is not queried, and its output rows hold zeros (counts) and -1 (near_d2, near_row).  A
 * class outside [0, C) makes the point a QUERY ONLY: its own rows are computed and nobody counts it.  1 <= C <= HDY_SPATIAL_MAX_CLASSES.
 * original row: where the point's outputs are written, 0 <= row < N, every row once (a row outside [0, N) is not written: any content is
 * memory-safe).
 *
 * cells.  A grid of ncx x ncy square cells of cell_units units, 1 <= ncx * ncy <= HDY_SPATIAL_MAX_CELLS; the cell of a present point is
 *     cell = min(y / cell_units, ncy - 1) * ncx + min(x / cell_units, ncx - 1)
 * (a coordinate beyond the grid falls into its last column / row, so that any content is memory-safe and the result below still holds).
 * hdy_spatial_cells and hdy_spatial_neighbors take pts SORTED by cell, absent points last; the order inside a cell is free.
 *
 * hdy_spatial_cells: cell_start int32 [ncx * ncy + 1], cell_start_elems = ncx * ncy + 1 exactly: entry c is the first sorted position whose
 * cell is >= c (absent points rank behind every cell), so the points of cell c are the positions cell_start[c] .. cell_start[c + 1] - 1 and the
 * last entry is the number of present points.  status int32 [1], status_elems = 1, written by the call: bit 0 is set when a point's cell is
 * lower than its predecessor's (pts is not in cell order, a present point behind an absent one included), else the word is 0.  The order is
 * checked no further; on unsorted pts every entry of cell_start still lies in [0, N].
 *
 * hdy_spatial_neighbors: radii is a HOST array of K int32 radii in units, 1 <= K <= HDY_SPATIAL_MAX_RADII, 1 <= r_1 < r_2 < ... < r_K <=
 * cell_units (read before the call returns).  For a present point p and every other present point q of class c in [0, C) — "other" by identity,
 * not by distance: a different point at the same position counts, with d2 = 0 —
 *     d2 = dx * dx + dy * dy   in int64,   q is within r of p when d2 <= r * r.
 *   counts   int32 [N][K][C]  counts[row p][k][c] = the q of class c within r_k (cumulative over the radii, not rings)
 *   near_d2  int64 [N][C]     the smallest d2 to a q of class c within r_K, -1 when there is none
 *   near_row int32 [N][C]     the original row of that q; among equal d2 the lowest original row; -1 when there is none
 * counts_elems = N * K * C, near_d2_elems = near_row_elems = N * C exactly.  Every entry of the three outputs is written (the rows of absent
 * points with 0 / -1), the caller's content does not matter.  One lane owns one row: no atomics.  The result is a pure function of the point
 * set: it does not depend on cell_units (any cell_units >= r_K), on the grid of the launch, on the order inside a cell or on repeats.  A point
 * tests the points of the (at most) nine cells around its own and no others.
 *
 * hdy_spatial_density: pts in ANY order.  grid int32 [gy][gx][C], grid_elems = gy * gx * C exactly (< 2^31): entry (fy, fx, c) counts the present
 * points of class c with y / g_units = fy and x / g_units = fx; points outside the gx x gy fields and query-only points are not counted.  The
 * call zeroes the grid itself; integer adds only.
 *
 * All passes: no allocation, no synchronisation, everything on `stream`.  All argument checks are made before any launch; HDY_EINVAL with a
 * message: null pointers where something would be read or written, misaligned pointers (pts 16 bytes; near_d2 8 bytes; the others 4 bytes),
 * negative counts, C or K out of range, radii that do not increase strictly from 1, r_K > cell_units, a grid with a side < 1 or more than
 * HDY_SPATIAL_MAX_CELLS cells, *_elems that differ from what the call reads or writes.  N = 0 launches nothing (the sizes are still checked;
 * the caller zeroes an empty density grid itself).  The dispatch log names the passes "spatial_cells", "spatial_neighbors", "spatial_density". */
#ifndef HDYOLO_SPATIAL_H
#define HDYOLO_SPATIAL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HDY_SPATIAL_REVISION 1
#define HDY_SPATIAL_SUBPIXEL 16
#define HDY_SPATIAL_MAX_CLASSES 16
#define HDY_SPATIAL_MAX_RADII 4
#define HDY_SPATIAL_MAX_COORD (1 << 26)
#define HDY_SPATIAL_MAX_CELLS (1 << 24)
int hdy_spatial_revision(void);
int hdy_spatial_cells(const int* pts, long long pts_elems, int N, int cell_units, int ncx, int ncy,
                      int* cell_start, long long cell_start_elems, int* status, long long status_elems, void* stream);
int hdy_spatial_neighbors(const int* pts, long long pts_elems, int N, const int* cell_start, long long cell_start_elems,
                          int cell_units, int ncx, int ncy, const int* radii, int K, int C,
                          int* counts, long long counts_elems, long long* near_d2, long long near_d2_elems,
                          int* near_row, long long near_row_elems, void* stream);
int hdy_spatial_density(const int* pts, long long pts_elems, int N, int g_units, int gx, int gy, int C,
                        int* grid, long long grid_elems, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HDYOLO_SPATIAL_H */
