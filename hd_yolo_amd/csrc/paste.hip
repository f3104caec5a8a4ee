// Instance masks pasted on the device: box-coordinate M x M probability patches -> image-space masks (hdy_paste_masks, the drop-in for
// torchvision's paste_masks_in_image) or one int32 label map of a canvas window (hdy_paste_label_map), and the pixel count of every label
// (hdy_label_areas).  Scalar fp32 / integer work bound by stores, atomics and L2; no MFMA, no LDS-DMA.
//
// The arithmetic is stated in include/hdyolo.h ("mask paste") and restated in tests/paste_ref.py; every product, sum and quotient below is one
// explicitly rounded operation (__fmul_rn / __fadd_rn / __fsub_rn / __fdiv_rn: no contraction into FMA), so the two agree bit for bit.
//
// paste_kernel<LABEL>: one workgroup per detection, one launch for all R.  The framed P x P patch (P = M + 2 padding <= 64) is staged in LDS.
// The box's pixel rectangle, clipped to the window, is walked in panels of up to PANEL x PANEL pixels: per panel the two axis tables (i0, l1
// per column and per row) are computed once by PANEL threads, then the lanes walk the panel row-major, so a wave's stores / atomics fall on
// contiguous bytes of one or a few map rows.  A nucleus-sized box is one panel; a box larger than the window is many, and a 1 x 1 box is one
// pixel of one lane.  Dense mode stores the value into the detection's own plane (zeroed by the entry point); label mode does an unsigned
// atomicMin of the row where value >= threshold on a map the entry point filled with 0xFF bytes: the lowest covering row wins whatever the
// arrival order, so repeats are bit-identical and no finishing pass exists.
//
// areas_kernel: a wave reads 64 consecutive map entries, finds the runs of equal labels with one ballot, and the first lane of a run adds the
// run's length to areas[label] (integer adds: exact and order-independent).  Background runs cost no atomic.
//
// Contract: no allocation, everything on the passed stream, no host synchronisation, no device-to-host copy; all argument checks before any launch.
#include "common.h"
#include "hdyolo.h"

namespace {

typedef unsigned long long u64;

constexpr int THREADS = 256;
constexpr int PANEL = 256;                       // panel side = threads: one table entry per thread and axis
constexpr int MAX_P = HDY_PASTE_MAX_M + 2;       // 64
constexpr float COORD_LIMIT = 1073741824.f;      // 2^30: expanded coordinates at or beyond it (or non-finite) paste nothing; keeps every index in int32

struct Args {
    const float* masks;
    const float* boxes;
    int M, pad, P;
    float scale, thr;
    int x0, y0, w, h;           // the window of the canvas that the output holds (dense mode: 0, 0, W, H)
    float* out;                 // dense: [R][h][w]
    unsigned* map;              // label: [h][w]
};

// source position of destination offset d along an axis of `sc` = P / extent: i0 and the weight of i0 + 1
__device__ __forceinline__ void axis_entry(float sc, int d, int P, int& i0, float& l1) {
    float s = __fsub_rn(__fmul_rn(sc, __fadd_rn((float)d, 0.5f)), 0.5f);
    s = s > 0.f ? s : 0.f;
    int i = (int)s;
    i = i < P - 1 ? i : P - 1;                   // (s < P - 0.5 by construction: a guard for the LDS index, never taken)
    i0 = i;
    l1 = __fsub_rn(s, (float)i);
}

template <bool LABEL>
__global__ __launch_bounds__(THREADS) void paste_kernel(const Args a) {
    __shared__ float patch[MAX_P * MAX_P];
    __shared__ int xi0[PANEL], yi0[PANEL];
    __shared__ float xl1[PANEL], yl1[PANEL];
    const int r = blockIdx.x, t = threadIdx.x;
    const int P = a.P;

    // ---- the integer box (every thread: four broadcast loads, no barrier before the uniform exits)
    const float x1 = a.boxes[4 * (size_t)r], y1 = a.boxes[4 * (size_t)r + 1], x2 = a.boxes[4 * (size_t)r + 2], y2 = a.boxes[4 * (size_t)r + 3];
    const float hx = __fmul_rn(__fmul_rn(__fsub_rn(x2, x1), 0.5f), a.scale), cx = __fmul_rn(__fadd_rn(x2, x1), 0.5f);
    const float hy = __fmul_rn(__fmul_rn(__fsub_rn(y2, y1), 0.5f), a.scale), cy = __fmul_rn(__fadd_rn(y2, y1), 0.5f);
    const float ex1 = __fsub_rn(cx, hx), ex2 = __fadd_rn(cx, hx), ey1 = __fsub_rn(cy, hy), ey2 = __fadd_rn(cy, hy);
    if (!(fabsf(ex1) < COORD_LIMIT && fabsf(ex2) < COORD_LIMIT && fabsf(ey1) < COORD_LIMIT && fabsf(ey2) < COORD_LIMIT)) return;   // NaN / inf too
    const int bx1 = (int)ex1, by1 = (int)ey1, bx2 = (int)ex2, by2 = (int)ey2;        // truncation toward zero
    const int bw = max(bx2 - bx1 + 1, 1), bh = max(by2 - by1 + 1, 1);                // |b| < 2^30: no overflow
    // clipped rectangle [cx0, cx1) x [cy0, cy1) in canvas coordinates
    const long long lx0 = max((long long)bx1, (long long)a.x0), lx1 = min((long long)bx1 + bw, (long long)a.x0 + a.w);
    const long long ly0 = max((long long)by1, (long long)a.y0), ly1 = min((long long)by1 + bh, (long long)a.y0 + a.h);
    if (lx0 >= lx1 || ly0 >= ly1) return;
    const int cx0 = (int)lx0, cx1 = (int)lx1, cy0 = (int)ly0, cy1 = (int)ly1;

    // ---- the framed patch
    const float* __restrict__ src = a.masks + (size_t)r * a.M * a.M;
    for (int i = t; i < P * P; i += THREADS) {
        const int py = i / P, px = i - py * P;
        const int my = py - a.pad, mx = px - a.pad;
        patch[i] = (my >= 0 && my < a.M && mx >= 0 && mx < a.M) ? src[my * a.M + mx] : 0.f;
    }
    const float scx = __fdiv_rn((float)P, (float)bw), scy = __fdiv_rn((float)P, (float)bh);

    for (int py0 = cy0; py0 < cy1; py0 += PANEL) {
        const int ph = min(PANEL, cy1 - py0);
        for (int px0 = cx0; px0 < cx1; px0 += PANEL) {
            const int pw = min(PANEL, cx1 - px0);
            __syncthreads();                                     // the previous panel's tables have been read (first panel: nothing pending)
            if (t < pw) axis_entry(scx, px0 + t - bx1, P, xi0[t], xl1[t]);
            if (t < ph) axis_entry(scy, py0 + t - by1, P, yi0[t], yl1[t]);
            __syncthreads();                                     // tables (and, the first time, the patch) are in LDS
            // row-major walk: thread t takes pixels t, t + 256, ... of the panel; (ry, rx) advances without a division
            const int qy = THREADS / pw, qx = THREADS - qy * pw;
            int ry = t / pw, rx = t - ry * pw;
            while (ry < ph) {
                const int ix0 = xi0[rx], iy0 = yi0[ry];
                const int ix1 = ix0 + (ix0 < P - 1 ? 1 : 0), iy1 = iy0 + (iy0 < P - 1 ? 1 : 0);
                const float wx1 = xl1[rx], wy1 = yl1[ry];
                const float wx0 = __fsub_rn(1.f, wx1), wy0 = __fsub_rn(1.f, wy1);
                const float top = __fadd_rn(__fmul_rn(wx0, patch[iy0 * P + ix0]), __fmul_rn(wx1, patch[iy0 * P + ix1]));
                const float bot = __fadd_rn(__fmul_rn(wx0, patch[iy1 * P + ix0]), __fmul_rn(wx1, patch[iy1 * P + ix1]));
                const float v = __fadd_rn(__fmul_rn(wy0, top), __fmul_rn(wy1, bot));
                const long long at = (long long)(py0 + ry - a.y0) * a.w + (px0 + rx - a.x0);
                if constexpr (LABEL) {
                    if (v >= a.thr) atomicMin(&a.map[at], (unsigned)r);
                } else {
                    a.out[(long long)r * a.h * a.w + at] = v;
                }
                rx += qx;
                ry += qy;
                if (rx >= pw) { rx -= pw; ++ry; }
            }
        }
    }
}

__global__ __launch_bounds__(THREADS) void areas_kernel(const int* __restrict__ map, long long n, int* __restrict__ areas, int R) {
    const int lane = threadIdx.x & 63;
    const long long stride = (long long)gridDim.x * THREADS;
    for (long long base = (long long)blockIdx.x * THREADS + (threadIdx.x - lane); base < n; base += stride) {       // wave-uniform
        const long long i = base + lane;
        const int v = i < n ? map[i] : -1;
        const int prev = __shfl_up(v, 1);
        const bool head = lane == 0 || v != prev;
        const u64 heads = __ballot(head);
        if (head && v >= 0 && v < R) {
            const u64 rest = lane == 63 ? 0ull : heads >> (lane + 1);
            atomicAdd(&areas[v], rest ? __ffsll((unsigned long long)rest) : 64 - lane);
        }
    }
}

// the checks shared by the two paste entry points; on success *P and *scale are set
int check_common(const char* who, const float* masks, int R, int M, int padding, const float* boxes) {
    HDY_ARG(R >= 0, "%s: negative row count R=%d", who, R);
    HDY_ARG(M >= HDY_PASTE_MIN_M && M <= HDY_PASTE_MAX_M, "%s: M=%d outside [%d, %d]", who, M, HDY_PASTE_MIN_M, HDY_PASTE_MAX_M);
    HDY_ARG(padding == 0 || padding == 1, "%s: padding=%d (0 or 1)", who, padding);
    HDY_ARG(R == 0 || (masks && boxes), "%s: null masks or boxes pointer", who);
    HDY_ARG((((uintptr_t)masks | (uintptr_t)boxes) & 3) == 0, "%s: misaligned pointer", who);
    return HDY_OK;
}

Args make_args(const float* masks, int M, int padding, const float* boxes) {
    Args a = {};
    a.masks = masks; a.boxes = boxes; a.M = M; a.pad = padding; a.P = M + 2 * padding;
    a.scale = (float)a.P / (float)M;             // one IEEE division = the fp32 rounding of the double quotient for integers this small
    return a;
}

}  // namespace

extern "C" {

int hdy_paste_masks(const float* masks, int R, int M, int padding, const float* boxes, float* out, long long out_elems, int H, int W, void* stream) {
    const char* who = "paste_masks";
    if (int rc = check_common(who, masks, R, M, padding, boxes)) return rc;
    HDY_ARG(H >= 1 && W >= 1 && H <= HDY_PASTE_MAX_SIDE && W <= HDY_PASTE_MAX_SIDE, "%s: canvas %d x %d outside [1, %d]", who, H, W, HDY_PASTE_MAX_SIDE);
    const unsigned __int128 need = (unsigned __int128)R * (unsigned)H * (unsigned)W;
    HDY_ARG(out_elems >= 0 && (unsigned __int128)out_elems == need, "%s: out_elems=%lld, the call writes R * H * W = %d * %d * %d", who, out_elems, R, H, W);
    HDY_ARG(R == 0 || out, "%s: null out pointer", who);
    HDY_ARG(((uintptr_t)out & 3) == 0, "%s: misaligned pointer", who);
    if (R == 0) return HDY_OK;
    Args a = make_args(masks, M, padding, boxes);
    a.x0 = 0; a.y0 = 0; a.w = W; a.h = H; a.out = out; a.thr = 0.f;
    hipStream_t st = (hipStream_t)stream;
    HDY_CHECKED(hdy_memset_async(who, out, 0, (size_t)out_elems * 4, st));
    hipLaunchKernelGGL(paste_kernel<false>, dim3(R), dim3(THREADS), 0, st, a);
    HDY_LAUNCH_CHECK(who);
    hdy_note_dispatch("paste_dense");
    return HDY_OK;
}

int hdy_paste_label_map(const float* masks, int R, int M, int padding, const float* boxes, float threshold, int x0, int y0, int* map,
                        long long map_elems, int h, int w, void* stream) {
    const char* who = "paste_label_map";
    if (int rc = check_common(who, masks, R, M, padding, boxes)) return rc;
    HDY_ARG(h >= 1 && w >= 1 && h <= HDY_PASTE_MAX_SIDE && w <= HDY_PASTE_MAX_SIDE, "%s: window %d x %d outside [1, %d]", who, h, w, HDY_PASTE_MAX_SIDE);
    HDY_ARG(x0 >= -HDY_PASTE_MAX_SIDE && x0 <= HDY_PASTE_MAX_SIDE && y0 >= -HDY_PASTE_MAX_SIDE && y0 <= HDY_PASTE_MAX_SIDE,
            "%s: window origin (%d, %d) outside [-%d, %d]", who, x0, y0, HDY_PASTE_MAX_SIDE, HDY_PASTE_MAX_SIDE);
    HDY_ARG(map_elems == (long long)h * w, "%s: map_elems=%lld, the call writes h * w = %d * %d", who, map_elems, h, w);
    HDY_ARG(map, "%s: null map pointer", who);
    HDY_ARG(((uintptr_t)map & 3) == 0, "%s: misaligned pointer", who);
    HDY_ARG(threshold == threshold, "%s: threshold is NaN", who);
    Args a = make_args(masks, M, padding, boxes);
    a.x0 = x0; a.y0 = y0; a.w = w; a.h = h; a.map = (unsigned*)map; a.thr = threshold;
    hipStream_t st = (hipStream_t)stream;
    HDY_CHECKED(hdy_memset_async(who, map, 0xFF, (size_t)map_elems * 4, st));
    if (R > 0) hipLaunchKernelGGL(paste_kernel<true>, dim3(R), dim3(THREADS), 0, st, a);
    HDY_LAUNCH_CHECK(who);
    hdy_note_dispatch("paste_label");
    return HDY_OK;
}

int hdy_label_areas(const int* map, long long map_elems, int* areas, int R, void* stream) {
    const char* who = "label_areas";
    HDY_ARG(R >= 0 && map_elems >= 0, "%s: negative count (R=%d, map_elems=%lld)", who, R, map_elems);
    HDY_ARG((map || map_elems == 0) && (areas || R == 0), "%s: null map or areas pointer", who);
    HDY_ARG((((uintptr_t)map | (uintptr_t)areas) & 3) == 0, "%s: misaligned pointer", who);
    if (R == 0) return HDY_OK;
    hipStream_t st = (hipStream_t)stream;
    HDY_CHECKED(hdy_memset_async(who, areas, 0, (size_t)R * 4, st));
    if (map_elems > 0) {
        const long long blocks = (map_elems + THREADS - 1) / THREADS;
        hipLaunchKernelGGL(areas_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(THREADS), 0, st, map, map_elems, areas, R);
    }
    HDY_LAUNCH_CHECK(who);
    hdy_note_dispatch("label_areas");
    return HDY_OK;
}

}  // extern "C"
