// What csrc/augment.hip (pixels, boxes) and csrc/augment_masks.hip (instance masks) share: the cell table's layout, the canvas -> source map of
// the image kernel, the box pipeline behind a canvas box, the one-workgroup compaction and the argument checks of a mosaic.  include/hdyolo.h
// states every formula; tests/augment_ref.py and tests/augment_mask_ref.py restate them on the CPU.
#pragma once
#include <hip/hip_runtime.h>

#include "common.h"
#include "hdyolo.h"

namespace {

constexpr int AUG_ROWS = 4;                 // output rows per workgroup; patch >= AUG_ROWS, so a band touches at most two mosaic rows
constexpr int AUG_KMAX = 8;                 // largest mosaic side
constexpr int CELL_WORDS = HDY_AUG_CELL_BYTES / 4;
constexpr int W_SRC = 0, W_INV = 1, W_FLAGS = 10, W_FWD = 11, W_SCALE = 20, W_LUT = 24;
constexpr unsigned F_HFLIP = 1, F_VFLIP = 2, F_TRANSPOSE = 4, F_HSV = 8, F_PERSP = 16;
constexpr int BOX_MAX_CELLS = 4096;         // B * k * k of one hdy_augment_boxes call
constexpr int BOX_MAX_PER_TILE = 65536;
constexpr int MASK_BACKGROUND = 0xFFFF;     // value of an instance map's unowned pixels; object indices are below it
constexpr int MASK_REC_WORDS = 8;           // one extents record: count, umin, umax, vmin, vmax, area_img, 0, 0
constexpr int MASK_SIDE = 28;

// canvas pixel (u, v) of a cell (flips already undone) -> its source position in 1/32 pixel; false: NaN or far away
__device__ __forceinline__ bool canvas_to_q(const unsigned* cp, int u, int v, int* qx, int* qy) {
    const float fu = (float)u, fv = (float)v;
    const float* m = (const float*)cp + W_INV;
    float sx = __fadd_rn(__fadd_rn(__fmul_rn(m[0], fu), __fmul_rn(m[1], fv)), m[2]);
    float sy = __fadd_rn(__fadd_rn(__fmul_rn(m[3], fu), __fmul_rn(m[4], fv)), m[5]);
    if (cp[W_FLAGS] & F_PERSP) {
        const float sw = __fadd_rn(__fadd_rn(__fmul_rn(m[6], fu), __fmul_rn(m[7], fv)), m[8]);
        sx = __fdiv_rn(sx, sw);
        sy = __fdiv_rn(sy, sw);
    }
    const float tx = __fmul_rn(sx, 32.0f), ty = __fmul_rn(sy, 32.0f);
    const float LIM = 16777216.0f;
    if (!(tx >= -LIM && tx <= LIM && ty >= -LIM && ty <= LIM)) return false;
    *qx = __float2int_rn(tx);
    *qy = __float2int_rn(ty);
    return true;
}

// exclusive prefix of v over the 1024 threads of the workgroup (thread order) and the total; wsum: int [17] of LDS
__device__ __forceinline__ int block_scan_1024(int v, int* wsum, int* total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(inc, d);
        if (lane >= d) inc += t;
    }
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        for (int i = 0; i < 16; ++i) {
            const int t = wsum[i];
            wsum[i] = s;
            s += t;
        }
        wsum[16] = s;
    }
    __syncthreads();
    const int res = wsum[wv] + inc - v;
    *total = wsum[16];
    __syncthreads();
    return res;
}

__device__ __forceinline__ float clip_f(float v, float hi) { return fminf(fmaxf(v, 0.0f), hi); }

// the canvas box of a source box: its four corners through the cell's forward matrix, clipped to the canvas (include/hdyolo.h, "Targets")
__device__ __forceinline__ void corner_box(const float* bx, const unsigned* cp, int P, float* nb) {
    const float* F = (const float*)cp + W_FWD;
    const unsigned flags = cp[W_FLAGS];
    const float fP = (float)P;
    const float xs[4] = {bx[0], bx[0], bx[2], bx[2]}, ys[4] = {bx[1], bx[3], bx[3], bx[1]};
    float x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f;
    bool anyx = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float X = __fadd_rn(__fadd_rn(__fmul_rn(xs[j], F[0]), __fmul_rn(ys[j], F[1])), F[2]);
        float Y = __fadd_rn(__fadd_rn(__fmul_rn(xs[j], F[3]), __fmul_rn(ys[j], F[4])), F[5]);
        if (flags & F_PERSP) {
            const float Wd = __fadd_rn(__fadd_rn(__fmul_rn(xs[j], F[6]), __fmul_rn(ys[j], F[7])), F[8]);
            X = __fdiv_rn(X, Wd);
            Y = __fdiv_rn(Y, Wd);
        }
        X = clip_f(X, fP);
        Y = clip_f(Y, fP);
        anyx = anyx || X != 0.0f;
        x1 = j ? fminf(x1, X) : X;
        x2 = j ? fmaxf(x2, X) : X;
        y1 = j ? fminf(y1, Y) : Y;
        y2 = j ? fmaxf(y2, Y) : Y;
    }
    if (!anyx) x1 = y1 = x2 = y2 = 0.0f;                       // Mask.box: all-zero x gives a zero box
    nb[0] = x1; nb[1] = y1; nb[2] = x2; nb[3] = y2;
}

// a canvas box nb of the source box bx through the candidate test (area ratio above area_thr), the flips, mosaic and crop offsets, the two
// filters and the normalisation; false: dropped
__device__ __forceinline__ bool box_tail(const float* bx, const float* nb, float area_thr, const unsigned* cp, int r, int c, int P, int S, int cx,
                                         int cy, float* o) {
    const float sc = ((const float*)cp)[W_SCALE];
    const unsigned flags = cp[W_FLAGS];
    const float fP = (float)P, fS = (float)S;
    float x1 = nb[0], y1 = nb[1], x2 = nb[2], y2 = nb[3];
    const float eps = 1e-16f;
    const float w1 = __fsub_rn(__fmul_rn(bx[2], sc), __fmul_rn(bx[0], sc)), h1 = __fsub_rn(__fmul_rn(bx[3], sc), __fmul_rn(bx[1], sc));
    const float w2 = __fsub_rn(x2, x1), h2 = __fsub_rn(y2, y1);
    const float ar = fmaxf(__fdiv_rn(w2, __fadd_rn(h2, eps)), __fdiv_rn(h2, __fadd_rn(w2, eps)));
    const float ratio = __fdiv_rn(__fmul_rn(w2, h2), __fadd_rn(__fmul_rn(w1, h1), eps));
    if (!(w2 > 2.0f && h2 > 2.0f && ratio > area_thr && ar < 100.0f)) return false;
    if (flags & F_HFLIP) {
        const float a = fabsf(__fsub_rn(x2, fP)), e = fabsf(__fsub_rn(x1, fP));
        x1 = a; x2 = e; y1 = fabsf(y1); y2 = fabsf(y2);
    }
    if (flags & F_VFLIP) {
        const float a = fabsf(__fsub_rn(y2, fP)), e = fabsf(__fsub_rn(y1, fP));
        y1 = a; y2 = e; x1 = fabsf(x1); x2 = fabsf(x2);
    }
    if (flags & F_TRANSPOSE) {
        float t = x1; x1 = y1; y1 = t;
        t = x2; x2 = y2; y2 = t;
    }
    const float ox = __fsub_rn((float)(c * P), (float)cx), oy = __fsub_rn((float)(r * P), (float)cy);   // exact: integers below 2^24
    x1 = __fadd_rn(x1, ox); x2 = __fadd_rn(x2, ox);
    y1 = __fadd_rn(y1, oy); y2 = __fadd_rn(y2, oy);
    if (!(x1 < x2 && y1 < y2)) return false;                   // the crop's filter looks at the UNCLIPPED box: it removes nothing here
    x1 = clip_f(x1, fS); x2 = clip_f(x2, fS);
    y1 = clip_f(y1, fS); y2 = clip_f(y2, fS);
    if (!(x1 < __fsub_rn(x2, 10.0f) && y1 < __fsub_rn(y2, 10.0f))) return false;
    o[0] = __fdiv_rn(x1, fS); o[1] = __fdiv_rn(y1, fS); o[2] = __fdiv_rn(x2, fS); o[3] = __fdiv_rn(y2, fS);
    return true;
}

// what the compaction needs beyond boxes when some rows carry an instance mask (hdy_augment_boxes_masks); unused without
struct MaskRows {
    const unsigned char* has_mask;          // [M]
    const int* ws;                          // extents records [cell][pitch][MASK_REC_WORDS]
    int pitch;
    int* out_ref;                           // [cap][2] = (cell, object of the cell's tile)
    int* total;                             // [1] = rows written
};

// One workgroup of 1024 threads.  The candidates (image, cell in (r, c) order, source order) are walked 1024 at a time; each chunk's keep
// flags are prefix-summed, so the compact order is the candidate order and repeats give the same bits.  No atomics.  MASKS: a row with
// has_mask takes its canvas box from its extents record and the 0.01 candidate test.
template <bool MASKS>
__global__ __launch_bounds__(1024) void augment_boxes_kernel(const float* __restrict__ bank_boxes, const long long* __restrict__ bank_labels,
                                                             const long long* __restrict__ offsets, int n, int M, const unsigned* __restrict__ cells,
                                                             const int* __restrict__ crop, int B, int P, int k, int S, float* __restrict__ out_boxes,
                                                             long long* __restrict__ out_labels, float* __restrict__ out_img, int cap,
                                                             int* __restrict__ counts, int* __restrict__ overflow, MaskRows mk) {
    __shared__ int cstart[BOX_MAX_CELLS + 1];                  // first candidate of a cell
    __shared__ int cpos[BOX_MAX_CELLS + 1];                    // rows kept before a cell's first candidate
    __shared__ int wsum[17];
    const int k2 = k * k, ncell = B * k2, tid = threadIdx.x;
    int loc[4], s = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ci = 4 * tid + j;
        int cnt = 0;
        if (ci < ncell) {
            const int b = ci / k2, cx = crop[2 * b], cy = crop[2 * b + 1];
            const int src = (int)cells[(size_t)ci * CELL_WORDS + W_SRC];
            if (src >= 0 && src < n && cx >= 0 && cy >= 0 && cx <= k * P - S && cy <= k * P - S) {
                const long long lo = offsets[src], hi = offsets[src + 1];
                if (lo >= 0 && hi >= lo && hi <= M) cnt = (int)min(hi - lo, (long long)BOX_MAX_PER_TILE);
            }
        }
        loc[j] = cnt;
        s += cnt;
    }
    int T;
    int e = block_scan_1024(s, wsum, &T);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        cstart[4 * tid + j] = e;
        e += loc[j];
    }
    if (tid == 1023) cstart[BOX_MAX_CELLS] = e;
    __syncthreads();
    int base = 0;
    for (int t0 = 0; t0 < T; t0 += 1024) {
        const int t = t0 + tid;
        int keep = 0, ci = 0, b = 0, w = 0;
        long long row = 0;
        float o[4];
        if (t < T) {
            int lo = 0, hi = ncell - 1;                        // the cell with cstart[ci] <= t < cstart[ci + 1]
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (cstart[mid + 1] <= t) lo = mid + 1;
                else hi = mid;
            }
            ci = lo;
            b = ci / k2;
            const int j = ci - b * k2, r = j / k, c = j - r * k;
            const unsigned* cp = cells + (size_t)ci * CELL_WORDS;
            w = t - cstart[ci];
            row = offsets[(int)cp[W_SRC]] + w;
            const f32x4 v = *(const f32x4*)(bank_boxes + row * 4);
            const float bx[4] = {v[0], v[1], v[2], v[3]};
            float nb[4], thr = 0.1f;
            if (MASKS && w < mk.pitch && w < MASK_BACKGROUND && mk.has_mask[row]) {
                const int* rec = mk.ws + ((size_t)ci * mk.pitch + w) * MASK_REC_WORDS;
                const i32x4 q = *(const i32x4*)rec;            // count, umin, umax, vmin
                const int vmax = rec[4];
                const bool any = q[0] > 0;
                nb[0] = any ? (float)q[1] : 0.0f;
                nb[1] = any ? (float)q[3] : 0.0f;
                nb[2] = any ? (float)(q[2] + 1) : 0.0f;
                nb[3] = any ? (float)(vmax + 1) : 0.0f;
                thr = 0.01f;
            } else {
                corner_box(bx, cp, P, nb);
            }
            keep = box_tail(bx, nb, thr, cp, r, c, P, S, crop[2 * b], crop[2 * b + 1], o) ? 1 : 0;
        }
        int total;
        const int ex = block_scan_1024(keep, wsum, &total);
        if (t < T && t == cstart[ci]) cpos[ci] = base + ex;
        if (keep && base + ex < cap) {
            const size_t d = (size_t)(base + ex);
            f32x4 wv = {o[0], o[1], o[2], o[3]};
            *(f32x4*)(out_boxes + d * 4) = wv;
            out_labels[d] = bank_labels[row];
            out_img[d] = (float)b;
            if (MASKS) {
                mk.out_ref[2 * d] = ci;
                mk.out_ref[2 * d + 1] = w;
            }
        }
        base += total;
    }
    __syncthreads();
    if (tid == 0) {
        cpos[ncell] = base;
        for (int ci = ncell - 1; ci >= 0; --ci)
            if (cstart[ci + 1] == cstart[ci]) cpos[ci] = cpos[ci + 1];       // a cell without candidates starts where the next one does
        overflow[0] = base > cap ? 1 : 0;
        if (MASKS) mk.total[0] = min(base, cap);
    }
    __syncthreads();
    for (int b = tid; b < B; b += 1024) counts[b] = cpos[(b + 1) * k2] - cpos[b * k2];
}

inline bool mosaic_args_ok(const void* cells, int n_cells, const void* crop, int B, int patch, int k, int img_size, const char* who) {
    if (!cells || !crop) {
        hdy_set_error("%s: null cell table or crop offsets", who);
        return false;
    }
    if (B <= 0 || k < 1 || k > AUG_KMAX) {
        hdy_set_error("%s: batch of %d images, mosaic side %d (1 .. %d)", who, B, k, AUG_KMAX);
        return false;
    }
    if (patch < AUG_ROWS || patch > (1 << 15) || img_size <= 0 || img_size > k * patch) {
        hdy_set_error("%s: patch %d (%d .. 32768), img_size %d (1 .. k * patch = %d)", who, patch, AUG_ROWS, img_size, k * patch);
        return false;
    }
    if ((long long)n_cells != (long long)B * k * k) {
        hdy_set_error("%s: the cell table holds %d cells, B * k * k = %lld expected", who, n_cells, (long long)B * k * k);
        return false;
    }
    if (((uintptr_t)cells & 3) || ((uintptr_t)crop & 3)) {
        hdy_set_error("%s: cell table or crop offsets not 4-byte aligned", who);
        return false;
    }
    return true;
}

}  // namespace
