// What the passes over a slide's int32 label map share (measure.hip, outline.hip, texture.hip): the argument checks of the map window, of the
// extent table and of the 8-bit image window under the map, a label's extent clamped into the window, the ownership test of a map entry, the
// address of a pixel and the grid of a walk over the labels.  Everything is local to the including file.  The bounds are arguments: every
// public header states its own (HDY_*_MAX_WINDOW, HDY_*_MAX_SIDE).  The null and alignment checks stay with the entry points, which each name
// their own set of pointers.
#pragma once
#include "common.h"

namespace {

enum { FLAG_EMPTY = 1, FLAG_SIDE = 2 };          // a label's box: nothing of it inside the window, a side above the pass's bound

// the map window: sides in [1, max_window], map_elems = h * w in 64 bits
int check_map(const char* who, long long map_elems, int h, int w, int max_window) {
    HDY_ARG(map_elems >= 0, "%s: negative count (map_elems=%lld)", who, map_elems);
    HDY_ARG(h >= 1 && w >= 1 && h <= max_window && w <= max_window, "%s: window %d x %d outside [1, %d]", who, h, w, max_window);
    HDY_ARG(map_elems == (long long)h * w, "%s: map_elems=%lld, the call reads h * w = %d * %d", who, map_elems, h, w);
    return HDY_OK;
}

// verb: "reads" or "writes", what the call does with the extent table
int check_extent(const char* who, long long extent_elems, int R, const char* verb) {
    HDY_ARG(R >= 0 && extent_elems >= 0, "%s: negative count (R=%d, extent_elems=%lld)", who, R, extent_elems);
    HDY_ARG(extent_elems == 4ll * R, "%s: extent_elems=%lld, the call %s 4 * R = 4 * %d", who, extent_elems, verb, R);
    return HDY_OK;
}

// the h x w window at (x0, y0) of the image: the last byte a pass reads, the third of the window's last pixel, lies below image_bytes (128-bit)
int check_image(const char* who, int h, int w, long long image_bytes, long long row_stride, int pixel_stride, int x0, int y0) {
    HDY_ARG(pixel_stride == 3 || pixel_stride == 4, "%s: pixel_stride=%d (3 or 4)", who, pixel_stride);
    HDY_ARG(row_stride > 0, "%s: row_stride=%lld must be positive", who, row_stride);
    HDY_ARG(x0 >= 0 && y0 >= 0, "%s: negative image window origin (%d, %d)", who, x0, y0);
    HDY_ARG(image_bytes >= 0, "%s: negative image_bytes=%lld", who, image_bytes);
    const unsigned __int128 last = (unsigned __int128)((long long)y0 + h - 1) * (unsigned long long)row_stride +
                                   (unsigned __int128)((long long)x0 + w - 1) * (unsigned)pixel_stride + 2;
    HDY_ARG(last < (unsigned __int128)image_bytes, "%s: the image window (%d, %d) + %d x %d at row_stride=%lld, pixel_stride=%d leaves image_bytes=%lld",
            who, x0, y0, w, h, row_stride, pixel_stride, image_bytes);
    return HDY_OK;
}

// workgroups of a grid-stride walk over `rows` labels of which a workgroup takes per_block at a time (its lanes or its waves), at most cap
unsigned label_blocks(int rows, int per_block, int cap) {
    const long long blocks = ((long long)rows + per_block - 1) / per_block;
    return (unsigned)(blocks < cap ? blocks : cap);
}

// the image under the map: entry (i, j) of the map window is the pixel (y0 + i, x0 + j), three colour bytes at a pixel stride of 3 or 4
struct Image {
    const unsigned char* img;
    long long row_stride;
    int ps, x0, y0;
    __host__ __device__ __forceinline__ const unsigned char* pixel(int i, int j) const {
        return img + ((long long)y0 + i) * row_stride + ((long long)x0 + j) * ps;
    }
};

// the label's extent clamped into the window; FLAG_EMPTY (bw = bh = 0) / FLAG_SIDE (a side above max_side) when there is nothing to do
struct Box { int x0, y0, bw, bh, flag; };
__host__ __device__ __forceinline__ Box clamped_box(const int* __restrict__ extent, int r, int h, int w, int max_side) {
    const int* e = extent + 4 * (size_t)r;
    const int ex0 = e[0], ey0 = e[1], ex1 = e[2], ey1 = e[3];
    Box b;
    b.x0 = ex0 > 0 ? ex0 : 0;
    b.y0 = ey0 > 0 ? ey0 : 0;
    const int x1 = ex1 < w - 1 ? ex1 : w - 1, y1 = ey1 < h - 1 ? ey1 : h - 1;
    // x0 may be up to 2^31 - 1 and x1 down to -2^31: compare before subtracting
    b.flag = (x1 < b.x0 || y1 < b.y0) ? FLAG_EMPTY : 0;
    b.bw = b.flag ? 0 : x1 - b.x0 + 1;
    b.bh = b.flag ? 0 : y1 - b.y0 + 1;
    if (!b.flag && (b.bw > max_side || b.bh > max_side)) b.flag = FLAG_SIDE;
    return b;
}

// entry (i, j) lies inside the window and holds label r
__host__ __device__ __forceinline__ bool owns(const int* __restrict__ map, int h, int w, int i, int j, int r) {
    return (unsigned)i < (unsigned)h && (unsigned)j < (unsigned)w && map[(long long)i * w + j] == r;
}

}  // namespace
