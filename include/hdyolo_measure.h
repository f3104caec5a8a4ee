/* hdyolo_measure.h — extension header of libhdyolo_hip.so: per-label measurements of a slide label map (csrc/measure.hip).
 *
 * An extension header declares entry points that are not part of the numbered ABI of hdyolo.h: it carries a revision of its own
 * (HDY_MEASURE_REVISION, hdy_measure_revision()), is bound by hd_yolo_amd/_ext.py and leaves HDY_ABI_VERSION alone.  The conventions are
 * hdyolo.h's: plain pointers and sizes, caller-owned buffers, everything on `stream`, 0 = ok, < 0 = invalid argument (hdy_last_error() says
 * which), > 0 = a hipError_t.
 *
 * ---- label measurement: one streaming pass over an int32 label map and the 8-bit slide under it ------------------------------------------
 * hdy_label_measure continues where hdy_paste_label_map and hdy_label_areas (hdyolo.h, "mask paste") stop: from the map of a window and,
 * optionally, the slide's 8-bit pixels it leaves per label a row of exact integer sums, from which position, size, second moments, outline
 * length, border contact and stain statistics follow (hd_yolo_amd/measure.py: nucleus_table).  The reference has no counterpart: it pastes
 * per image on the host (val_nuclei.py:169-176) and measures nothing.
 *
 * map int32 [h][w], map_elems = h * w exactly (64-bit: the product may pass 2^31); entry (i, j) is row i, column j and belongs to label
 * r = map[i][j] when 0 <= r < R.  Every other value (-1, 0x7fffffff, labels at or above R, ...) is background: any map content is memory-safe.
 * origin int32 [R][2] = (ox, oy) per label in window coordinates, or NULL = zeros: the point the moments are taken about, so that they stay
 * small (the caller passes the truncated top-left corner of the detection's box).
 * image NULL: columns 8-13 are zero.  Otherwise the 8-bit pixel of entry (i, j) starts at byte (y0 + i) * row_stride + (x0 + j) * pixel_stride
 * of `image`; its bytes 0, 1, 2 are R, G, B; pixel_stride is 3 or 4, row_stride > 0, x0 >= 0, y0 >= 0, and the last byte the call can read,
 * (y0 + h - 1) * row_stride + (x0 + w - 1) * pixel_stride + 2, lies below image_bytes (the pointer travels with its size).
 *
 * sums int64 [R][HDY_MEASURE_COLS], sums_elems = HDY_MEASURE_COLS * R exactly.  With dx = j - ox, dy = i - oy, over the label's entries, in 64-bit
 * two's complement (modulo 2^64):
 *   col 0          n                      (equal to hdy_label_areas)
 *   col 1, 2       sum dx, sum dy
 *   col 3, 4, 5    sum dx^2, sum dy^2, sum dx * dy
 *   col 6          boundary edges: per entry, the number of its four neighbours (i +- 1, j), (i, j +- 1) that lie outside the window or hold a
 *                  raw value different from r
 *   col 7          of those, the ones that lie outside the window
 *   col 8, 9, 10   sum R, sum G, sum B
 *   col 11, 12, 13 sum R^2, sum G^2, sum B^2
 * extent int32 [R][4] = {min j, min i, max j, max i}, extent_elems = 4 * R exactly; a label that owns nothing keeps {w, h, -1, -1}.
 *
 * Both outputs are initialised by the call: the caller's content does not matter.  Integer adds and integer minima / maxima only, so the result
 * is a pure function of the inputs: no dependence on arrival order, grid size or repeats.  No allocation, no synchronisation, everything on
 * `stream`.  All argument checks are made before any launch; HDY_EINVAL with a message: null pointers where something would be read or
 * written, misaligned pointers (sums 8 bytes; map, origin, extent 4 bytes), negative counts, sides outside [1, HDY_MEASURE_MAX_SIDE], *_elems
 * that differ from what the call reads or writes, a pixel_stride other than 3 or 4, row_stride <= 0, a negative x0 / y0, an image window that
 * leaves image_bytes.  R = 0 launches nothing.  The dispatch log names the pass "label_measure". */
#ifndef HDYOLO_MEASURE_H
#define HDYOLO_MEASURE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HDY_MEASURE_REVISION 1
#define HDY_MEASURE_COLS 14
#define HDY_MEASURE_MAX_SIDE (1 << 29)
int hdy_measure_revision(void);
int hdy_label_measure(const int* map, long long map_elems, int h, int w,
                      const unsigned char* image, long long image_bytes, long long row_stride, int pixel_stride, int x0, int y0,
                      const int* origin, long long* sums, long long sums_elems, int* extent, long long extent_elems, int R, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HDYOLO_MEASURE_H */
