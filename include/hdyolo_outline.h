/* hdyolo_outline.h — extension header of libhdyolo_hip.so: the outline polygon and the convex hull of every label of a slide label map
 * (csrc/outline.hip).
 *
 * An extension header declares entry points that are not part of the numbered ABI of hdyolo.h: it carries a revision of its own
 * (HDY_OUTLINE_REVISION, hdy_outline_revision()), is bound by hd_yolo_amd/_ext.py and leaves HDY_ABI_VERSION alone.  The conventions are
 * hdyolo.h's: plain pointers and sizes, caller-owned buffers, everything on `stream`, 0 = ok, < 0 = invalid argument (hdy_last_error() says
 * which), > 0 = a hipError_t.
 *
 * ---- from the label map and the extents of hdy_label_measure to polygons and hull descriptors ----------------------------------------------
 * The three passes continue where hdy_label_measure (hdyolo_measure.h) stops: its `extent` says where every label lies, and from the map and
 * that box they leave the label's outline as a polygon (count, then write, with the caller's prefix sum between them) and the descriptors
 * that need a convex hull (area, perimeter, the two Feret diameters).  The reference has no counterpart: it pastes per image on the host and
 * measures nothing.  The arithmetic below is this project's own, restated in tests/outline_ref.py.
 *
 * map int32 [h][w], map_elems = h * w exactly, 1 <= h, w <= HDY_OUTLINE_MAX_WINDOW; entry (i, j) is row i, column j and belongs to label
 * r = map[i][j] when 0 <= r < R.  Every other value is background, and so is everything outside the window: any map content is memory-safe.
 * extent int32 [R][4] = {min j, min i, max j, max i} as hdy_label_measure leaves it, extent_elems = 4 * R exactly.  Any extent content is
 * memory-safe: the box is clamped into the window first, (bx0, by0, bx1, by1) = (max(min j, 0), max(min i, 0), min(max j, w - 1),
 * min(max i, h - 1)), bw = bx1 - bx0 + 1, bh = by1 - by0 + 1, and every label gets one of the
 *   flags   0  measured
 *           1  the clamped box is empty (bw < 1 or bh < 1): a label that owns nothing
 *           2  bw or bh above HDY_OUTLINE_MAX_SIDE: the label is skipped
 *           4  the extent was not this map's (stated per pass below)
 * A flagged label has zeros in every other column.
 *
 * geometry.  Pixels are unit squares: pixel (i, j) covers [j, j + 1] x [i, i + 1].  Vertices are lattice corners (x, y) with 0 <= x <= w and
 * 0 <= y <= h; x runs to the right and y DOWN, as on screen.
 *
 * outline of label r.  Let s = (i0, j0) be the first entry of r in row i0 = by0, scanning the columns bx0 .. bx1, and K the 4-connected
 * component of {map == r} that contains s.  The outline is the outer boundary of K, followed crack by crack (a crack is a unit pixel edge):
 * it starts at corner (j0, i0) heading +x along the top edge of s and keeps K on its right (clockwise on screen).  Having passed a crack in
 * direction d it looks at the two pixels ahead, A on its right and B on its left: A not r -> turn right; A and B both r -> turn left; else
 * straight on.  So at a corner where K touches itself only diagonally the walk stays with its own pixel (foreground is 4-connected,
 * background 8-connected), and pixels of r that hang on K by a corner only are not part of it.  The walk ends when it is back at (j0, i0)
 * heading +x.  Only corners where the direction changes are vertices, the start corner being vertex 0; V >= 4 and V is even.  With this
 * orientation  sum_k (x_k * y_{k+1} - x_{k+1} * y_k)  (indices modulo V) is positive and equals twice the number of pixels of K and its holes,
 * a hole being a part of the background that does not reach the outside of K through 8-connectivity.
 * flag 4 of the outline: no entry of r in row by0 between bx0 and bx1; or the entry above s or to the left of s is r (s is not the label's
 * first entry); or the walk has not closed after cap = bw * (bh + 1) + bh * (bw + 1) cracks, the number of lattice edges of the clamped
 * box (a walk inside the box passes every edge at most once, so one that takes more has left the box); or the sum above is not
 * positive (the walk went round a hole).  With the extent of hdy_label_measure on the same map none of these happens.
 *
 * hdy_label_outline_count: counts int64 [R][4] = {V, the sum above (twice the enclosed area), the number of cracks L, flags}, counts_elems =
 * 4 * R exactly; every entry is written.
 *
 * hdy_label_outline_write: offsets int64 [R + 1], offsets_elems = R + 1 exactly, the exclusive prefix sum of counts[:, 0] (the caller makes
 * it); verts int32 [total][2] = (x, y), verts_elems = 2 * total exactly (total = 0: verts may be NULL); status int32 [1], written by the call.
 * The pass walks again and writes vertex k of label r to row offsets[r] + k.  Every row index is checked against offsets[r], offsets[r + 1]
 * and total before the store; a label whose range offsets[r + 1] - offsets[r] differs from its V (0 for a flagged label) gets no store
 * beyond its range, and bit 0 of status is set, else the word is 0.  Rows outside the ranges of offsets are never touched.
 *
 * hdy_label_hull: the convex hull of ALL pixel squares of label r inside its clamped box: fragments are included and holes ignored, which
 * is what solidity conventionally means.  flag 4 of the hull: no entry of r in row by0 between bx0 and bx1.
 *   hull_i int64 [R][4]   {hull vertices H, twice the hull area, the squared maximum Feret diameter = the largest squared distance between
 *                         two hull corners, flags}, exact
 *   hull_f double [R][2]  {hull perimeter, minimum Feret diameter = the smallest caliper width: the minimum over hull edges of the largest
 *                         distance of a hull corner from the edge's line}; 0 for a flagged label
 * hull_i_elems = 4 * R, hull_f_elems = 2 * R exactly.  A single pixel gives H = 4, 2, 2, perimeter 4, minimum Feret diameter 1.  Collinear
 * corners are no hull vertices.  The hull is that of, per lattice row y of the box, the leftmost and the rightmost corner of the label's
 * pixels above and below y; the integer columns and every cross product (below 2^22 under the side bound) are exact, the perimeter is a sum
 * of correctly rounded square roots of exact integers in a fixed order, the minimum Feret diameter one such root and one division.
 *
 * All passes: no allocation, no synchronisation, everything on `stream`; the result is a pure function of the inputs.  All argument checks
 * are made before any launch; HDY_EINVAL with a message: null pointers where something would be read or written, misaligned pointers
 * (counts, offsets, hull_i, hull_f 8 bytes; the others 4 bytes), negative counts, sides outside [1, HDY_OUTLINE_MAX_WINDOW], *_elems that
 * differ from what the call reads or writes, an odd verts_elems.  R = 0 launches nothing (the sizes are still checked; the caller zeroes
 * status itself).  The dispatch log names the passes "label_outline_count", "label_outline_write", "label_hull". */
#ifndef HDYOLO_OUTLINE_H
#define HDYOLO_OUTLINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HDY_OUTLINE_REVISION 1
#define HDY_OUTLINE_MAX_SIDE 1024
#define HDY_OUTLINE_MAX_WINDOW (1 << 29)
int hdy_outline_revision(void);
int hdy_label_outline_count(const int* map, long long map_elems, int h, int w, const int* extent, long long extent_elems, int R,
                            long long* counts, long long counts_elems, void* stream);
int hdy_label_outline_write(const int* map, long long map_elems, int h, int w, const int* extent, long long extent_elems, int R,
                            const long long* offsets, long long offsets_elems, int* verts, long long verts_elems,
                            int* status, void* stream);
int hdy_label_hull(const int* map, long long map_elems, int h, int w, const int* extent, long long extent_elems, int R,
                   long long* hull_i, long long hull_i_elems, double* hull_f, long long hull_f_elems, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HDYOLO_OUTLINE_H */
