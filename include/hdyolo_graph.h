/* hdyolo_graph.h — extension header of libhdyolo_hip.so: the cell graph of a slide's nuclei (csrc/graph.hip).
 *
 * The fourth extension header (see hdyolo_spatial.h for what an extension header is): a revision of its own (HDY_GRAPH_REVISION,
 * hdy_graph_revision()), bound by hd_yolo_amd/_ext.py, HDY_ABI_VERSION left alone.  The conventions are hdyolo.h's: plain pointers and sizes,
 * caller-owned buffers, everything on `stream`, 0 = ok, < 0 = invalid argument (hdy_last_error() says which), > 0 = a hipError_t.
 *
 * ---- the k nearest neighbours of every nucleus ---------------------------------------------------------------------------------------------
 * The reference has no counterpart (it relates no detection to another); the arithmetic below is this project's own, all of it integer,
 * restated in tests/graph_ref.py.
 *
 * points and cells are exactly those of hdyolo_spatial.h.  pts int32 [N][4] = (x, y, class, original row), pts_elems = 4 * N exactly, 16-byte
 * aligned, x and y in units of 1 / HDY_SPATIAL_SUBPIXEL pixel.  A point with a negative coordinate is ABSENT.  A grid of ncx x ncy square cells
 * of cell_units units, 1 <= ncx * ncy <= HDY_SPATIAL_MAX_CELLS,
 *     cell = min(y / cell_units, ncy - 1) * ncx + min(x / cell_units, ncx - 1)
 * (a coordinate beyond the grid falls into its last column / row); pts is SORTED by cell, absent points last, the order inside a cell free;
 * cell_start int32 [ncx * ncy + 1] is what the unchanged hdy_spatial_cells wrote for this pts and this grid.
 *
 * hdy_graph_knn.  For a present point p the CANDIDATES are the other present points q with class >= 0 — "other" by identity, not by distance:
 * a different point at the same position counts, with d2 = 0 — that satisfy
 *     d2 = dx * dx + dy * dy <= max_radius * max_radius     in int64.
 * A negative class makes a point a QUERY ONLY: it gets neighbours and is nobody's.  There is no upper class limit here.  The NEIGHBOURS of p
 * are the first k candidates in ascending (d2, original row) order (fewer when there are fewer candidates).  1 <= k <= HDY_GRAPH_MAX_K,
 * max_radius >= 1 units.
 *   nbr_row   int32 [N][k]   the original rows of the neighbours of row p, nearest first, padded with -1
 *   nbr_d2    int64 [N][k]   their d2, padded with -1
 *   nbr_count int32 [N]      how many there are (0 .. k)
 * nbr_row_elems = nbr_d2_elems = N * k, nbr_count_elems = N exactly.  Outputs are indexed by original row; every entry is written whatever the
 * caller left there; the rows of absent points hold -1 / -1 / 0.  (An original row outside [0, N) is not written: any content of pts is
 * memory-safe.)  One lane owns one row: no atomics.  The result is a pure function of the point set: it does not depend on cell_units, on the
 * grid, on the launch, on the order inside a cell or on repeats.
 *
 * the search.  A lane visits the cells around its own cell (cx, cy) ring by ring: ring t = the cells at Chebyshev distance exactly t, t = 0, 1,
 * ...  The two outer rows of a ring (cy - t and cy + t, columns cx - t .. cx + t) are one contiguous range of pts each, the rows between give
 * the two single cells cx - t and cx + t; everything is clipped at the grid and every range is clamped into [0, N].
 *
 *   Claim: after ring t every present point q the lane has not visited satisfies d(p, q) > t * cell_units.
 *   Proof.  q lies in a cell (qx, qy) with |qx - cx| > t or |qy - cy| > t; take the x axis, y is alike.  Write c for cell_units.  The cell rule
 *   gives v >= (cell index of v) * c for every present coordinate v, clamped or not (clamping only lowers the index), and v < (index + 1) * c
 *   for every coordinate whose index is not the last one of its axis (such a coordinate is not clamped).
 *     qx >= cx + t + 1: then cx is not the last column, so p.x < (cx + 1) * c, and q.x >= qx * c: q.x - p.x > (qx - cx - 1) * c >= t * c.
 *     qx <= cx - t - 1: then qx is not the last column, so q.x < (qx + 1) * c <= (cx - t) * c, and p.x >= cx * c: p.x - q.x > t * c.
 *   So |dx| > t * c or |dy| > t * c, hence d > t * c.  The clamped last column / row needs no special case: a point beyond the grid is only
 *   ever further out than its cell says, on the side where the proof uses a lower bound.
 *
 * A lane stops after ring t when
 *   (a) it holds k candidates and the d2 of its k-th is <= (t * cell_units)^2: every unvisited point is strictly further than its k-th, so no
 *       tie is open; or
 *   (b) t * cell_units >= max_radius: every unvisited point is further than max_radius; or
 *   (c) the ring has left the grid on all four sides (cx - t <= 0, cx + t >= ncx - 1, cy - t <= 0, cy + t >= ncy - 1): nothing is unvisited.
 * The last ring is therefore at most R = ceil(max_radius / cell_units), and the call requires R <= HDY_GRAPH_MAX_RINGS: every loop bound is a
 * checked constant (R, 2 * R - 1 inner rows, k list slots) or a range clamped into [0, N]; no content of pts or cell_start can make a loop run
 * on.  On a cell_start that is not this pts's the result is wrong but every access stays inside the buffers.
 *
 * hdy_graph_mutual.  nbr_row int32 [N][k] (nbr_row_elems = N * k), mutual int32 [N][k] (mutual_elems = N * k): entry (p, s) is 1 when
 * q = nbr_row[p][s] lies in [0, N) and p occurs among nbr_row[q][0 .. k - 1], else 0.  One lane per (p, s), no atomics; any content of nbr_row
 * is memory-safe.
 *
 * Both passes: no allocation, no synchronisation, everything on `stream`.  All argument checks are made before any launch; HDY_EINVAL with a
 * message: null pointers where something would be read or written, misaligned pointers (pts 16 bytes; nbr_d2 8 bytes; the others 4 bytes),
 * negative counts, k outside [1, HDY_GRAPH_MAX_K], max_radius < 1, cell_units < 1, a grid with a side < 1 or more than HDY_SPATIAL_MAX_CELLS
 * cells, more than HDY_GRAPH_MAX_RINGS rings, *_elems that differ from what the call reads or writes.  N = 0 launches nothing (the sizes are
 * still checked).  The dispatch log names the passes "graph_knn" and "graph_mutual". */
#ifndef HDYOLO_GRAPH_H
#define HDYOLO_GRAPH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HDY_GRAPH_REVISION 1
#define HDY_GRAPH_MAX_K 16
#define HDY_GRAPH_MAX_RINGS 16
int hdy_graph_revision(void);
int hdy_graph_knn(const int* pts, long long pts_elems, int N, const int* cell_start, long long cell_start_elems,
                  int cell_units, int ncx, int ncy, int k, int max_radius,
                  int* nbr_row, long long nbr_row_elems, long long* nbr_d2, long long nbr_d2_elems,
                  int* nbr_count, long long nbr_count_elems, void* stream);
int hdy_graph_mutual(const int* nbr_row, long long nbr_row_elems, int N, int k, int* mutual, long long mutual_elems, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HDYOLO_GRAPH_H */
