// Instance masks through the device augmentation of csrc/augment.hip: a tile bank that carries an instance map (uint16 per pixel: the index of
// the owning object within its tile, 0xFFFF background) yields, per kept object, the box of its warped mask and a 28 x 28 mask target.
// Reference call sites: metayolo/datasets.py random_projective (:329-337: the box of a masked object is the box of its warped mask, candidate
// test at area_thr 0.01), the flips / mosaic / crop of the masks, target_to_tensors (:482-494: crop to the rounded box, bilinear resize to 28 x
// 28, zero below 25 pixels).  The reference warps polygons and calls cv2; the arithmetic here is this library's own: a canvas pixel belongs to
// the warped mask when the source pixel NEAREST to its source position (the image kernel's own canvas -> source map) is owned by the object.
// include/hdyolo.h states every formula; tests/augment_mask_ref.py restates them over the whole canvas, and the two agree bit for bit.
//
// Three launches behind hdy_augment_tiles_u8:
//   extents      one wave per candidate (cell, object): the lanes walk a canvas region that contains every member, a wave reduction gives the
//                member count, the extents and the count inside the image; lane 0 stores the 32-byte record.  No atomics, no LDS.
//   boxes_masks  the compaction of hdy_augment_boxes (augment_common.h) with the masked rows' boxes taken from their records.
//   targets      one workgroup per kept row (the row count is read on the device): 28 x 28 bilinear taps of the image-space mask.
#include <hip/hip_runtime.h>

#include "augment_common.h"

namespace {

struct MapView {
    const unsigned short* base;             // dense [n][H][W]
    int n, H, W;
};

// is canvas pixel (u, v) of the cell a member of the warped mask of object w of the cell's source tile
__device__ __forceinline__ bool mask_member(const MapView& mp, const unsigned* cp, int u, int v, int w) {
    int qx, qy;
    if (!canvas_to_q(cp, u, v, &qx, &qy)) return false;
    const int xn = (qx + 16) >> 5, yn = (qy + 16) >> 5;        // the nearest source pixel
    const int src = (int)cp[W_SRC];
    if (src < 0 || src >= mp.n || xn < 0 || xn >= mp.W || yn < 0 || yn >= mp.H) return false;
    return (int)mp.base[((size_t)src * mp.H + yn) * mp.W + xn] == w;
}

// the candidate (cell ci, object w): false when the cell owns nothing, the object does not exist or carries no mask
struct Candidate {
    int b, r, c, cx, cy;
    long long row;
};

__device__ __forceinline__ bool candidate(int ci, int w, int n, int M, const unsigned* cells, const int* crop, const long long* offsets,
                                          const unsigned char* has_mask, int pitch, int P, int k, int S, Candidate* cd, bool* exists) {
    const int k2 = k * k;
    cd->b = ci / k2;
    const int j = ci - cd->b * k2;
    cd->r = j / k;
    cd->c = j - cd->r * k;
    cd->cx = crop[2 * cd->b];
    cd->cy = crop[2 * cd->b + 1];
    *exists = false;
    if (!(cd->cx >= 0 && cd->cy >= 0 && cd->cx <= k * P - S && cd->cy <= k * P - S)) return false;
    const int src = (int)cells[(size_t)ci * CELL_WORDS + W_SRC];
    if (src < 0 || src >= n) return false;
    const long long lo = offsets[src], hi = offsets[src + 1];
    if (!(lo >= 0 && hi >= lo && hi <= M)) return false;
    if (w < 0 || w >= pitch || w >= min(hi - lo, (long long)BOX_MAX_PER_TILE)) return false;
    *exists = true;
    cd->row = lo + w;
    return w < MASK_BACKGROUND && has_mask[cd->row] != 0;
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = min(v, __shfl_xor(v, d));
    return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = max(v, __shfl_xor(v, d));
    return v;
}

// A canvas region [u0, u1] x [v0, v1] that contains every member of the object with source box bx.  A member's nearest source pixel lies in the
// box grown to pixel edges (TileBank validates that), so its source position lies in [floor(x1) - 0.52, ceil(x2) - 0.5]; the region is the
// bounding box of the forward-warped corners of [floor(x1) - 1.5, ceil(x2) + 0.5] (a full source pixel of slack on each side, against the
// rounding of the two fp32 matrices, which are inverses of each other only to about 1e-6 of a coordinate), grown by two canvas pixels.  A
// projective map sends the rectangle to the quadrilateral of its corners only while the denominator keeps its sign over it: when it comes near
// zero at a corner, or a corner is not finite, the region is the whole canvas.
__device__ __forceinline__ void member_region(const float* bx, const unsigned* cp, int P, int* u0, int* u1, int* v0, int* v1) {
    const float* F = (const float*)cp + W_FWD;
    const float gx[2] = {floorf(bx[0]) - 1.5f, ceilf(bx[2]) + 0.5f}, gy[2] = {floorf(bx[1]) - 1.5f, ceilf(bx[3]) + 0.5f};
    float lox = 0.f, hix = 0.f, loy = 0.f, hiy = 0.f;
    bool whole = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float x = gx[j & 1], y = gy[j >> 1];
        float X = x * F[0] + y * F[1] + F[2], Y = x * F[3] + y * F[4] + F[5];
        if (cp[W_FLAGS] & F_PERSP) {
            const float Wd = x * F[6] + y * F[7] + F[8];
            if (!(Wd >= 0.05f)) whole = true;
            X = X / Wd;
            Y = Y / Wd;
        }
        lox = j ? fminf(lox, X) : X;
        hix = j ? fmaxf(hix, X) : X;
        loy = j ? fminf(loy, Y) : Y;
        hiy = j ? fmaxf(hiy, Y) : Y;
    }
    const float BIG = 1.0e6f;
    if (!(lox >= -BIG && hix <= BIG && loy >= -BIG && hiy <= BIG)) whole = true;              // NaN included
    if (whole) {
        *u0 = 0; *v0 = 0; *u1 = P - 1; *v1 = P - 1;
        return;
    }
    *u0 = max((int)floorf(lox) - 2, 0);
    *v0 = max((int)floorf(loy) - 2, 0);
    *u1 = min((int)ceilf(hix) + 2, P - 1);
    *v1 = min((int)ceilf(hiy) + 2, P - 1);
}

__global__ __launch_bounds__(256) void mask_extents_kernel(MapView mp, const float* __restrict__ bank_boxes, const unsigned char* __restrict__ has_mask,
                                                           const long long* __restrict__ offsets, int M, const unsigned* __restrict__ cells,
                                                           const int* __restrict__ crop, int ncell, int P, int k, int S, int* __restrict__ ws,
                                                           int pitch) {
    const long long gw = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);                     // one wave per (cell, object): all tests below are wave-uniform
    const int lane = threadIdx.x & 63;
    if (gw >= (long long)ncell * pitch) return;
    const int ci = (int)(gw / pitch), w = (int)(gw - (long long)ci * pitch);
    Candidate cd;
    bool exists;
    const bool masked = candidate(ci, w, mp.n, M, cells, crop, offsets, has_mask, pitch, P, k, S, &cd, &exists);
    if (!exists) return;
    int cnt = 0, area = 0, umin = P, umax = -1, vmin = P, vmax = -1;
    if (masked) {
        const unsigned* cp = cells + (size_t)ci * CELL_WORDS;
        const unsigned flags = cp[W_FLAGS];
        const f32x4 bv = *(const f32x4*)(bank_boxes + cd.row * 4);
        const float bx[4] = {bv[0], bv[1], bv[2], bv[3]};
        int u0, u1, v0, v1;
        member_region(bx, cp, P, &u0, &u1, &v0, &v1);
        const int rw = u1 - u0 + 1, rh = v1 - v0 + 1;
        const int npx = rw > 0 && rh > 0 ? rw * rh : 0;                                      // <= 2^30
        const int offx = cd.c * P - cd.cx, offy = cd.r * P - cd.cy;
        for (int idx = lane; idx < npx; idx += 64) {
            const int dv = idx / rw, u = u0 + idx - dv * rw, v = v0 + dv;
            if (!mask_member(mp, cp, u, v, w)) continue;
            ++cnt;
            umin = min(umin, u); umax = max(umax, u);
            vmin = min(vmin, v); vmax = max(vmax, v);
            int iu = (flags & F_HFLIP) ? P - 1 - u : u, iv = (flags & F_VFLIP) ? P - 1 - v : v;
            if (flags & F_TRANSPOSE) { const int t = iu; iu = iv; iv = t; }
            const int ox = iu + offx, oy = iv + offy;
            area += ox >= 0 && ox < S && oy >= 0 && oy < S;
        }
        cnt = wave_sum(cnt);
        area = wave_sum(area);
        umin = wave_min(umin); umax = wave_max(umax);
        vmin = wave_min(vmin); vmax = wave_max(vmax);
        if (cnt == 0) umin = umax = vmin = vmax = 0;
    } else {
        umin = umax = vmin = vmax = 0;
    }
    if (lane == 0) {
        int* rec = ws + ((size_t)ci * pitch + w) * MASK_REC_WORDS;
        const i32x4 a = {cnt, umin, umax, vmin}, b = {vmax, area, 0, 0};
        *(i32x4*)rec = a;
        *(i32x4*)(rec + 4) = b;
    }
}

__global__ __launch_bounds__(256) void mask_targets_kernel(MapView mp, const unsigned char* __restrict__ has_mask, const long long* __restrict__ offsets,
                                                           int M, const unsigned* __restrict__ cells, const int* __restrict__ crop, int ncell, int P,
                                                           int k, int S, const int* __restrict__ ws, int pitch, const float* __restrict__ out_boxes,
                                                           const int* __restrict__ out_ref, const int* __restrict__ total,
                                                           float* __restrict__ out_masks) {
    const int row = (int)blockIdx.x;
    if (row >= total[0]) return;
    const int ci = out_ref[2 * row], w = out_ref[2 * row + 1];
    float* om = out_masks + (size_t)row * (MASK_SIDE * MASK_SIDE);
    Candidate cd;
    bool exists;
    bool live = ci >= 0 && ci < ncell && candidate(ci, w, mp.n, M, cells, crop, offsets, has_mask, pitch, P, k, S, &cd, &exists);
    int x1 = 0, y1 = 0, wd = 0, ht = 0;
    if (live) {
        live = ws[((size_t)ci * pitch + w) * MASK_REC_WORDS + 5] >= 25;                      // area_img: fewer pixels are an artifact
        const f32x4 bv = *(const f32x4*)(out_boxes + (size_t)row * 4);
        const float fS = (float)S;
        x1 = min(max(__float2int_rn(__fmul_rn(bv[0], fS)), 0), S);
        y1 = min(max(__float2int_rn(__fmul_rn(bv[1], fS)), 0), S);
        wd = min(max(__float2int_rn(__fmul_rn(bv[2], fS)), 0), S) - x1;
        ht = min(max(__float2int_rn(__fmul_rn(bv[3], fS)), 0), S) - y1;
        live = live && wd >= 1 && ht >= 1;
    }
    if (!live) {
        for (int e = threadIdx.x; e < MASK_SIDE * MASK_SIDE; e += 256) om[e] = 0.0f;
        return;
    }
    const unsigned* cp = cells + (size_t)ci * CELL_WORDS;
    const unsigned flags = cp[W_FLAGS];
    const float stepx = __fdiv_rn((float)wd, (float)MASK_SIDE), stepy = __fdiv_rn((float)ht, (float)MASK_SIDE);
    // the image-space mask at image pixel (x, y): zero outside the object's cell
    auto tap = [&](int x, int y) -> float {
        const int X = x + cd.cx, Y = y + cd.cy;
        if (X / P != cd.c || Y / P != cd.r) return 0.0f;
        int u = X - cd.c * P, v = Y - cd.r * P;
        if (flags & F_TRANSPOSE) { const int t = u; u = v; v = t; }
        if (flags & F_VFLIP) v = P - 1 - v;
        if (flags & F_HFLIP) u = P - 1 - u;
        return mask_member(mp, cp, u, v, w) ? 1.0f : 0.0f;
    };
    for (int e = threadIdx.x; e < MASK_SIDE * MASK_SIDE; e += 256) {
        const int i = e / MASK_SIDE, j = e - i * MASK_SIDE;
        const float fx = __fsub_rn(__fmul_rn((float)j + 0.5f, stepx), 0.5f), fy = __fsub_rn(__fmul_rn((float)i + 0.5f, stepy), 0.5f);
        int x0 = (int)floorf(fx), y0 = (int)floorf(fy);
        float a = __fsub_rn(fx, (float)x0), b = __fsub_rn(fy, (float)y0);
        if (x0 < 0) { x0 = 0; a = 0.0f; }
        if (x0 >= wd - 1) { x0 = wd - 1; a = 0.0f; }
        if (y0 < 0) { y0 = 0; b = 0.0f; }
        if (y0 >= ht - 1) { y0 = ht - 1; b = 0.0f; }
        const int xb = min(x0 + 1, wd - 1), yb = min(y0 + 1, ht - 1);
        const float m00 = tap(x1 + x0, y1 + y0), m01 = tap(x1 + xb, y1 + y0), m10 = tap(x1 + x0, y1 + yb), m11 = tap(x1 + xb, y1 + yb);
        const float ia = __fsub_rn(1.0f, a), ib = __fsub_rn(1.0f, b);
        const float top = __fadd_rn(__fmul_rn(m00, ia), __fmul_rn(m01, a)), bot = __fadd_rn(__fmul_rn(m10, ia), __fmul_rn(m11, a));
        om[e] = __fadd_rn(__fmul_rn(top, ib), __fmul_rn(bot, b));
    }
}

bool mask_args_ok(const void* instances, int n, int H, int W, const void* ws, long long ws_bytes, int pitch, int n_cells, const char* who) {
    if (instances && (n <= 0 || H <= 0 || W <= 0 || H > (1 << 15) || W > (1 << 15))) {
        hdy_set_error("%s: instance map of %d tiles of %d x %d pixels", who, n, H, W);
        return false;
    }
    if ((uintptr_t)instances & 1) {
        hdy_set_error("%s: instance map not 2-byte aligned", who);
        return false;
    }
    if (pitch < 1 || pitch >= MASK_BACKGROUND + 1) {
        hdy_set_error("%s: workspace row pitch of %d objects (1 .. %d)", who, pitch, MASK_BACKGROUND);
        return false;
    }
    const long long need = (long long)n_cells * pitch * MASK_REC_WORDS * 4;
    if (ws_bytes < need) {
        hdy_set_error("%s: workspace of %lld bytes, %d cells x %d objects x 32 = %lld needed", who, ws_bytes, n_cells, pitch, need);
        return false;
    }
    if ((uintptr_t)ws & 15) {
        hdy_set_error("%s: workspace not 16-byte aligned", who);
        return false;
    }
    return true;
}

}  // namespace

extern "C" {

int hdy_augment_mask_extents(const uint16_t* instances, int n, int H, int W, const float* bank_boxes, const unsigned char* has_mask,
                             const long long* offsets, int M, const void* cells, int n_cells, const int* crop, int B, int patch, int k, int img_size,
                             void* ws, long long ws_bytes, int pitch, void* stream) {
    HDY_ARG(instances && bank_boxes && has_mask && offsets && ws, "augment_mask_extents: null pointer");
    HDY_ARG(M >= 0, "augment_mask_extents: bank with %d boxes", M);
    if (!mosaic_args_ok(cells, n_cells, crop, B, patch, k, img_size, "augment_mask_extents")) return HDY_EINVAL;
    if (!mask_args_ok(instances, n, H, W, ws, ws_bytes, pitch, n_cells, "augment_mask_extents")) return HDY_EINVAL;
    HDY_ARG(((uintptr_t)bank_boxes & 15) == 0, "augment_mask_extents: bank boxes not 16-byte aligned");
    const long long waves = (long long)n_cells * pitch;
    HDY_ARG((waves + 3) / 4 < (1LL << 31), "augment_mask_extents: grid too large");
    const MapView mp{instances, n, H, W};
    hipLaunchKernelGGL(mask_extents_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, (hipStream_t)stream, mp, bank_boxes, has_mask, offsets, M,
                       (const unsigned*)cells, crop, n_cells, patch, k, img_size, (int*)ws, pitch);
    hdy_note_dispatch("augment_mask_extents");
    HDY_LAUNCH_CHECK("augment_mask_extents");
    return HDY_OK;
}

int hdy_augment_boxes_masks(const float* bank_boxes, const long long* bank_labels, const unsigned char* has_mask, const long long* offsets, int n,
                            int M, const void* cells, int n_cells, const int* crop, int B, int patch, int k, int img_size, const void* ws,
                            long long ws_bytes, int pitch, float* out_boxes, long long* out_labels, float* out_img, int* out_ref, int cap,
                            int* counts, int n_counts, int* overflow, int* total, void* stream) {
    HDY_ARG(bank_boxes && bank_labels && has_mask && offsets && ws && out_boxes && out_labels && out_img && out_ref && counts && overflow && total,
            "augment_boxes_masks: null pointer");
    HDY_ARG(n > 0 && M >= 0, "augment_boxes_masks: bank of %d tiles with %d boxes", n, M);
    if (!mosaic_args_ok(cells, n_cells, crop, B, patch, k, img_size, "augment_boxes_masks")) return HDY_EINVAL;
    if (!mask_args_ok(nullptr, n, 0, 0, ws, ws_bytes, pitch, n_cells, "augment_boxes_masks")) return HDY_EINVAL;
    HDY_ARG(n_cells <= BOX_MAX_CELLS, "augment_boxes_masks: %d cells in one call (at most %d)", n_cells, BOX_MAX_CELLS);
    HDY_ARG(cap > 0, "augment_boxes_masks: capacity of %d rows", cap);
    HDY_ARG(n_counts == B, "augment_boxes_masks: %d counts for %d images", n_counts, B);
    HDY_ARG((((uintptr_t)bank_boxes | (uintptr_t)out_boxes) & 15) == 0, "augment_boxes_masks: box arrays are not 16-byte aligned");
    HDY_ARG((((uintptr_t)out_ref | (uintptr_t)total) & 3) == 0, "augment_boxes_masks: out_ref or total not 4-byte aligned");
    const MaskRows mk{has_mask, (const int*)ws, pitch, out_ref, total};
    hipLaunchKernelGGL(augment_boxes_kernel<true>, dim3(1), dim3(1024), 0, (hipStream_t)stream, bank_boxes, bank_labels, offsets, n, M,
                       (const unsigned*)cells, crop, B, patch, k, img_size, out_boxes, out_labels, out_img, cap, counts, overflow, mk);
    hdy_note_dispatch("augment_boxes_masks");
    HDY_LAUNCH_CHECK("augment_boxes_masks");
    return HDY_OK;
}

int hdy_augment_mask_targets(const uint16_t* instances, int n, int H, int W, const unsigned char* has_mask, const long long* offsets, int M,
                             const void* cells, int n_cells, const int* crop, int B, int patch, int k, int img_size, const void* ws,
                             long long ws_bytes, int pitch, const float* out_boxes, const int* out_ref, const int* total, int cap, float* out_masks,
                             long long out_elems, void* stream) {
    HDY_ARG(instances && has_mask && offsets && ws && out_boxes && out_ref && total && out_masks, "augment_mask_targets: null pointer");
    HDY_ARG(M >= 0, "augment_mask_targets: bank with %d boxes", M);
    if (!mosaic_args_ok(cells, n_cells, crop, B, patch, k, img_size, "augment_mask_targets")) return HDY_EINVAL;
    if (!mask_args_ok(instances, n, H, W, ws, ws_bytes, pitch, n_cells, "augment_mask_targets")) return HDY_EINVAL;
    HDY_ARG(cap > 0, "augment_mask_targets: capacity of %d rows", cap);
    const long long want = (long long)cap * MASK_SIDE * MASK_SIDE;
    HDY_ARG(out_elems == want, "augment_mask_targets: out_masks holds %lld elements, cap x 28 x 28 = %lld expected", out_elems, want);
    HDY_ARG((((uintptr_t)out_boxes | (uintptr_t)out_masks) & 15) == 0, "augment_mask_targets: out_boxes or out_masks not 16-byte aligned");
    HDY_ARG((((uintptr_t)out_ref | (uintptr_t)total) & 3) == 0, "augment_mask_targets: out_ref or total not 4-byte aligned");
    const MapView mp{instances, n, H, W};
    hipLaunchKernelGGL(mask_targets_kernel, dim3((unsigned)cap), dim3(256), 0, (hipStream_t)stream, mp, has_mask, offsets, M, (const unsigned*)cells,
                       crop, n_cells, patch, k, img_size, (const int*)ws, pitch, out_boxes, out_ref, total, out_masks);
    hdy_note_dispatch("augment_mask_targets");
    HDY_LAUNCH_CHECK("augment_mask_targets");
    return HDY_OK;
}

}  // extern "C"
