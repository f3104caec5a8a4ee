/* hdyolo_stain.h — extension header of libhdyolo_hip.so: stain estimation counts and recolouring of an 8-bit slide (csrc/stain.hip).
 *
 * An extension header declares entry points that are not part of the numbered ABI of hdyolo.h: it carries a revision of its own
 * (HDY_STAIN_REVISION, hdy_stain_revision()), is bound by hd_yolo_amd/_ext.py (the table of pixel extensions) and leaves HDY_ABI_VERSION
 * alone.  The conventions are hdyolo.h's: plain pointers and sizes, caller-owned buffers, everything on `stream`, 0 = ok, < 0 = invalid
 * argument (hdy_last_error() says which), > 0 = a hipError_t.  The reference has no counterpart; the arithmetic below is this project's own,
 * restated in tests/stain_ref.py, and hd_yolo_amd/stain.py makes the tables and turns the counts into stain vectors (Macenko et al. 2009).
 *
 * ---- common arguments ------------------------------------------------------------------------------------------------------------------------
 * slide, pitch_bytes, pixel_bytes, H, W: the 8-bit slide as hdy_slide_tissue_u8 takes it; pixel (x, y) starts at byte y * pitch_bytes +
 * x * pixel_bytes, its bytes 0, 1, 2 are R, G, B; pixel_bytes is 3 or 4; 1 <= H, W <= HDY_STAIN_MAX_SIDE.
 * x0, y0, w, h: a window inside the slide (0 <= x0, 1 <= w, x0 + w <= W, likewise in y).
 * step >= 1: the estimation passes visit the pixels (x0 + i * step, y0 + j * step) of the window, i < ceil(w / step), j < ceil(h / step);
 * at most 2^40 of them.
 * background, 0 .. 256: a pixel is tissue iff min(R, G, B) < background (the rule of hdy_slide_tissue_u8).  The estimation passes count
 * tissue pixels only.
 * ws, ws_bytes: a workspace of at least HDY_STAIN_MAX_BLOCKS * cells * 8 bytes, 8-byte aligned, where cells is the number of int64 values
 * the pass leaves (10; A + 1; 2 * B).  Its content before and after the call means nothing.
 *
 * Every pass sums in integers: per lane, then per wave and workgroup, then one int64 slab of `cells` values per workgroup in ws, which a
 * second small launch adds up in a fixed order.  No atomics on global memory, no floating point: the same input gives the same bits.  Every
 * output element is written by the call, whatever it held before.  No allocation, no synchronisation; all argument checks are made before
 * any launch: null or misaligned pointers (tables and hist 4 / 8 bytes), a geometry outside the bounds above, *_elems that differ from what
 * the call reads or writes, a workspace that is too small.
 *
 * ---- hdy_stain_moments_u8 --------------------------------------------------------------------------------------------------------------------
 * od int32 [256] in device memory, od_elems = 256: the optical density of a channel value in units of 2^-HDY_STAIN_OD_SHIFT, made on the
 * host as q(v) = round(2^10 * -log10((v + 1) / 256)), so q(255) = 0 and q(0) = 2466.  Entries must lie in [0, 4095] (the caller's duty: the
 * sums of any other table are unspecified, and any content is memory-safe).
 * sums int64 [10], sums_elems = 10: n, sum qR, sum qG, sum qB, sum qR^2, sum qR qG, sum qR qB, sum qG^2, sum qG qB, sum qB^2 over the
 * tissue pixels visited.
 *
 * ---- hdy_stain_angles_u8 ---------------------------------------------------------------------------------------------------------------------
 * lut int32 [2][3][256] in device memory, lut_elems = 1536; 1 <= A <= HDY_STAIN_MAX_BINS.  Per tissue pixel, in 32-bit two's complement,
 *   p_k = (lut[k][0][R] + lut[k][1][G] + lut[k][2][B]) >> HDY_STAIN_ANGLE_SHIFT      (arithmetic shift), k = 0, 1
 * If p_0 <= 0 the pixel adds one to skipped[0].  Otherwise s = p_0 + |p_1| and the pixel adds one to hist[bin],
 *   bin = floor(A * (s + p_1) / (2 * s))
 * which is monotone in the angle atan2(p_1, p_0) over (-pi/2, pi/2) and below A: p_1 < s.  The product is formed in unsigned 32 bits: with
 * |entry| <= 2^10 * 2466 (the projection of an optical density on a unit vector) |p| < 2^20 and A * (s + p_1) < 2^32.  Who checks the table:
 * the Python wrapper (ops.stain_angles reads the table's largest magnitude back once); the entry point cannot, the table being in device
 * memory, and does not synchronise.  For any table content the bin is clamped to A - 1, so the call is memory-safe; the counts of a table
 * beyond the bound are unspecified.
 * hist int64 [A], hist_elems = A; skipped int64 [1], skipped_elems = 1.
 *
 * ---- hdy_stain_levels_u8 ---------------------------------------------------------------------------------------------------------------------
 * lut int32 [2][3][256], lut_elems = 1536; 1 <= B <= HDY_STAIN_MAX_BINS.  Per tissue pixel and stain s = 0, 1
 *   level_s = min(max((lut[s][0][R] + lut[s][1][G] + lut[s][2][B]) >> HDY_STAIN_SHIFT, 0), B - 1)      (modulo 2^32, arithmetic shift)
 * the level rule of hdy_label_texture, over the whole window and per stain.  hist int64 [2][B], hist_elems = 2 * B: hist[s][level_s] += 1.
 *
 * ---- hdy_stain_apply_u8 ----------------------------------------------------------------------------------------------------------------------
 * Every pixel of the window is recoloured, background included (no step, no background argument).  dst is an image of the slide's H x W
 * with its own dst_pitch and dst_pixel_bytes (3 or 4); pixel (x, y) of the slide goes to pixel (x, y) of dst, and only the window is
 * written.  lut int32 [3][3][256], lut_elems = 2304; tone uint8 [T], tone_elems = T, 1 <= T <= HDY_STAIN_MAX_TONE.  Per channel c
 *   idx_c = min(max((lut[c][0][R] + lut[c][1][G] + lut[c][2][B]) >> HDY_STAIN_SHIFT, 0), T - 1),   out_c = tone[idx_c]
 * A fourth byte of dst is the source's where the source has one, 255 otherwise.  dst == slide with equal pitch and pixel size is allowed (a
 * pixel depends on itself only); any other overlap of the two images' bytes is refused (both pitches at most 2^32 bytes, so that the extents are exact).  Both tables (9 KB + T bytes) live in LDS.
 *
 * The dispatch log names the passes "stain_moments", "stain_angles", "stain_levels", "stain_apply". */
#ifndef HDYOLO_STAIN_H
#define HDYOLO_STAIN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HDY_STAIN_REVISION 1
#define HDY_STAIN_OD_SHIFT 10
#define HDY_STAIN_ANGLE_SHIFT 4
#define HDY_STAIN_SHIFT 16
#define HDY_STAIN_MAX_BINS 1024
#define HDY_STAIN_MAX_TONE 8192
#define HDY_STAIN_MAX_SIDE (1 << 29)
#define HDY_STAIN_MAX_BLOCKS 1024
int hdy_stain_revision(void);
int hdy_stain_moments_u8(const unsigned char* slide, long long pitch_bytes, int pixel_bytes, int H, int W, int x0, int y0, int w, int h, int step,
                         int background, const int* od, long long od_elems, long long* sums, long long sums_elems, void* ws, long long ws_bytes,
                         void* stream);
int hdy_stain_angles_u8(const unsigned char* slide, long long pitch_bytes, int pixel_bytes, int H, int W, int x0, int y0, int w, int h, int step,
                        int background, const int* lut, long long lut_elems, int A, long long* hist, long long hist_elems, long long* skipped,
                        long long skipped_elems, void* ws, long long ws_bytes, void* stream);
int hdy_stain_levels_u8(const unsigned char* slide, long long pitch_bytes, int pixel_bytes, int H, int W, int x0, int y0, int w, int h, int step,
                        int background, const int* lut, long long lut_elems, int B, long long* hist, long long hist_elems, void* ws,
                        long long ws_bytes, void* stream);
int hdy_stain_apply_u8(const unsigned char* slide, long long pitch_bytes, int pixel_bytes, int H, int W, int x0, int y0, int w, int h,
                       unsigned char* dst, long long dst_pitch, int dst_pixel_bytes, const int* lut, long long lut_elems,
                       const unsigned char* tone, long long tone_elems, int T, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HDYOLO_STAIN_H */
