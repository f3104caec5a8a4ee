/* hdyolo_texture.h — extension header of libhdyolo_hip.so: the grey-level histogram and the grey-level co-occurrence matrices (GLCM) of every
 * label of a slide label map (csrc/texture.hip).
 *
 * An extension header declares entry points that are not part of the numbered ABI of hdyolo.h: it carries a revision of its own
 * (HDY_TEXTURE_REVISION, hdy_texture_revision()), is bound by hd_yolo_amd/_ext.py and leaves HDY_ABI_VERSION alone.  The conventions are
 * hdyolo.h's: plain pointers and sizes, caller-owned buffers, everything on `stream`, 0 = ok, < 0 = invalid argument (hdy_last_error() says
 * which), > 0 = a hipError_t.
 *
 * ---- from the label map, the 8-bit slide and the extents of hdy_label_measure to level counts ----------------------------------------------
 * hdy_label_texture continues where hdy_label_measure (hdyolo_measure.h) stops: its `extent` says where every label lies, and from the map,
 * that box and the slide's pixels the pass leaves per label the histogram of quantised levels and one symmetric co-occurrence matrix per
 * offset, from which intensity statistics and the Haralick features follow (hd_yolo_amd/texture.py).  The reference has no counterpart: it
 * pastes per image on the host and measures nothing.  The arithmetic below is this project's own, restated in tests/texture_ref.py.
 *
 * map int32 [h][w], map_elems = h * w exactly, 1 <= h, w <= HDY_TEXTURE_MAX_WINDOW; entry (i, j) is row i, column j and belongs to label
 * r = map[i][j] when 0 <= r < R.  Every other value (-1, 0x7fffffff, labels at or above R, ...) is background, and so is everything outside
 * the window: any map content is memory-safe.
 * image (required): the 8-bit pixel of entry (i, j) starts at byte (y0 + i) * row_stride + (x0 + j) * pixel_stride of `image`; its bytes
 * 0, 1, 2 are R, G, B; pixel_stride is 3 or 4, row_stride > 0, x0 >= 0, y0 >= 0, and the last byte the call can read,
 * (y0 + h - 1) * row_stride + (x0 + w - 1) * pixel_stride + 2, lies below image_bytes (the pointer travels with its size).
 * extent int32 [R][4] = {min j, min i, max j, max i} as hdy_label_measure leaves it, extent_elems = 4 * R exactly.  Any extent content is
 * memory-safe: the box is clamped into the window first, (bx0, by0, bx1, by1) = (max(min j, 0), max(min i, 0), min(max j, w - 1),
 * min(max i, h - 1)), bw = bx1 - bx0 + 1, bh = by1 - by0 + 1, and every label of the call gets one of the
 *   flags   0  measured
 *           1  the clamped box is empty (bw < 1 or bh < 1): a label that owns nothing
 *           2  bw or bh above HDY_TEXTURE_MAX_SIDE: the label is skipped
 * A flagged label has zeros in hist and glcm.
 *
 * level of a pixel.  lut int32 [3][256] in device memory, lut_elems = 768 exactly; any content is memory-safe.  With
 *   t = lut[0][R] + lut[1][G] + lut[2][B]       in 32-bit two's complement (modulo 2^32)
 *   level = min(max(floor(t / 2^HDY_TEXTURE_SHIFT), 0), levels - 1)
 * and levels one of 8, 16, 32 (the largest is HDY_TEXTURE_MAX_LEVELS).  The pass knows nothing of stains: colour deconvolution, luma or a
 * single channel are all three per-channel tables (hd_yolo_amd/texture.py: stain_lut).
 *
 * offsets: a HOST array int [D][2] of (di, dj), read by the call before it returns; offsets_elems = 2 * D exactly, 1 <= D <=
 * HDY_TEXTURE_MAX_OFFSETS, |di|, |dj| <= HDY_TEXTURE_MAX_REACH, no offset is (0, 0).
 *
 * rows.  The call treats the labels row0 .. row0 + rows - 1, 0 <= row0, 0 <= rows, row0 + rows <= R, and the outputs are sized by `rows`, so
 * that a caller bounds the memory of the matrices by working through the labels in chunks.
 *
 * outputs, for output row q (label r = row0 + q), over the entries (i, j) of the clamped box with map[i][j] == r, a = level(i, j):
 *   hist int32 [rows][levels]                 hist[q][a] += 1
 *   glcm int32 [rows][D][levels][levels]      for every offset d, if (i + di, j + dj) lies inside the WINDOW (not only the box) and holds r,
 *                                             with b its level:  glcm[q][d][a][b] += 1  and  glcm[q][d][b][a] += 1
 *   flags int32 [rows]                        as above
 * hist_elems = rows * levels, glcm_elems = rows * D * levels * levels, flags_elems = rows exactly.  The matrix is the symmetric one: a pair
 * of equal levels adds 2 to the diagonal, and the sum of a matrix is twice the number of pairs.  Under the side bound a count is at most
 * 2 * 1024^2, so int32 is exact.  Every element of hist, glcm and flags is written by the call: the caller's content does not matter and no
 * separate init launch exists (a label belongs to one wave, which stores its finished matrices).
 *
 * Integer counting only, so the result is a pure function of the inputs: no dependence on arrival order, grid size or repeats.  No
 * allocation, no synchronisation, everything on `stream`.  All argument checks are made before any launch; HDY_EINVAL with a message that
 * names the argument: null pointers (offsets always; map, image, extent, lut, hist, glcm, flags where rows > 0), misaligned pointers (map,
 * extent, lut, offsets, hist, glcm, flags 4 bytes), negative counts, sides outside [1, HDY_TEXTURE_MAX_WINDOW], *_elems that differ from
 * what the call reads or writes, a pixel_stride other than 3 or 4, row_stride <= 0, a negative x0 / y0, an image window that leaves
 * image_bytes, levels other than 8, 16, 32, D outside [1, HDY_TEXTURE_MAX_OFFSETS], an offset beyond the reach or equal to (0, 0), a negative
 * row0 or rows, row0 + rows above R.  R = 0 or rows = 0 launches nothing (the checks are still made).  The dispatch log names the pass
 * "label_texture". */
#ifndef HDYOLO_TEXTURE_H
#define HDYOLO_TEXTURE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HDY_TEXTURE_REVISION 1
#define HDY_TEXTURE_MAX_SIDE 1024
#define HDY_TEXTURE_MAX_WINDOW (1 << 29)
#define HDY_TEXTURE_SHIFT 16
#define HDY_TEXTURE_MAX_LEVELS 32
#define HDY_TEXTURE_MAX_OFFSETS 4
#define HDY_TEXTURE_MAX_REACH 4
int hdy_texture_revision(void);
int hdy_label_texture(const int* map, long long map_elems, int h, int w,
                      const unsigned char* image, long long image_bytes, long long row_stride, int pixel_stride, int x0, int y0,
                      const int* extent, long long extent_elems, int R,
                      const int* lut, long long lut_elems, int levels,
                      const int* offsets, long long offsets_elems, int D,
                      int row0, int rows,
                      int* hist, long long hist_elems, int* glcm, long long glcm_elems, int* flags, long long flags_elems, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HDYOLO_TEXTURE_H */
