// Whole-slide inference from the slide as readers deliver it (8-bit HWC RGB / RGBA on the device): tile gather into the plan's input buffer,
// append of a batch's compacted detections to slide-wide arrays at a device-resident cursor, and per-tile tissue counts for blank-tile skipping.
// Reference call sites: the ROI protocol the reference composes around Detect.merge_outputs (metayolo/models/yolo_head.py:450-462) — the
// `/ 255` normalisation and the per-ROI crop of its loaders, and the per-ROI shift + cat of merge_outputs.  The tissue rule has no counterpart.
//
// All three are streaming kernels: no MFMA, no LDS-DMA.  The gather is an HBM stream dominated by its writes (8 B per pixel in bf16 against
// 3-4 B read): a thread handles FOUR pixels of one output row, reads their 12 / 16 source bytes as whole aligned dwords (funnel-shifted into
// place when the first byte is not dword aligned: 3-byte pixels, odd pitches and odd origins all stay on this path) and writes 16-byte
// vectors (two per thread in bf16, one per pixel in fp32).  Only groups that straddle a border — the zero frame of the stem layout, the
// slide's edges — take per-pixel byte loads.  An aligned dword that holds at least one byte of the slide lies inside the page of that byte,
// so the dword loads read at most 3 bytes beside the first / last pixel of a group and never another page.
#include <hip/hip_runtime.h>

#include "slide_common.h"
#include "hdyolo.h"

namespace {

// v / 255 correctly rounded to fp32 for the 256 values of a byte: made on the host with IEEE division, handed to the kernel by value.
// (v * (1.0f / 255) is another function: it differs from the quotient for 126 of the 256 values.)
struct U8Table {
    float v[256];
};

const U8Table& u8_table() {
    static const U8Table tab = [] {
        U8Table t;
        for (int i = 0; i < 256; ++i) {
            volatile float num = (float)i, den = 255.0f;      // volatile: the division is done as written, in fp32
            t.v[i] = num / den;
        }
        return t;
    }();
    return tab;
}

// one pixel of the stem layout: 4 x T = (r, g, b, 0) / 255
template <typename T>
__device__ __forceinline__ void store_px(T* o, unsigned px, const float* lut);
template <>
__device__ __forceinline__ void store_px<float>(float* o, unsigned px, const float* lut) {
    f32x4 v = {lut[px & 255], lut[(px >> 8) & 255], lut[(px >> 16) & 255], 0.f};
    *(f32x4*)o = v;
}
template <>
__device__ __forceinline__ void store_px<bf16_t>(bf16_t* o, unsigned px, const float* lut) {
    bf16x4 v = {from_f32<bf16_t>(lut[px & 255]), from_f32<bf16_t>(lut[(px >> 8) & 255]), from_f32<bf16_t>(lut[(px >> 16) & 255]), from_f32<bf16_t>(0.f)};
    *(bf16x4*)o = v;
}

// slide [H][pitch bytes] of PB-byte pixels -> out [count][th + 2 pad][tw + 2 pad][4] of T (the hdy_stem_prep layout: zero frame, zero 4th
// channel).  A block serves 256 four-pixel groups of one tile; bpt blocks per tile.  Pixels outside the slide are zero (lut[0] == 0).
template <typename T, int PB>
__global__ __launch_bounds__(256) void slide_tiles_stem_kernel(const unsigned char* __restrict__ slide, long long pitch, int H, int W,
                                                               const int* __restrict__ origins, int first, T* __restrict__ out, int th, int tw,
                                                               int pad, int bpt, U8Table tab) {
    __shared__ float lut[256];
    lut[threadIdx.x] = tab.v[threadIdx.x];
    __syncthreads();
    const int Hp = th + 2 * pad, Wp = tw + 2 * pad, G = (Wp + 3) >> 2;
    const int t = blockIdx.x / bpt;
    const int item = (blockIdx.x - t * bpt) * 256 + threadIdx.x;
    if (item >= Hp * G) return;
    const int hp = item / G, g = item - hp * G;
    const int x0 = origins[2 * (first + t)], y0 = origins[2 * (first + t) + 1];
    const int h = hp - pad, wp0 = 4 * g, w0 = wp0 - pad;
    const long long y = (long long)y0 + h, x = (long long)x0 + w0;
    unsigned px[4] = {0u, 0u, 0u, 0u};
    if (h >= 0 && h < th && y >= 0 && y < H) {
        const unsigned char* row = slide + y * pitch;           // 64-bit: y * pitch passes 2^32 on real slides
        if (w0 >= 0 && w0 + 4 <= tw && x >= 0 && x + 4 <= W) {
            load4<PB>(row + x * PB, px);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (w0 + j >= 0 && w0 + j < tw && x + j >= 0 && x + j < W) px[j] = load1(row + (x + j) * PB);
        }
    }
    T* o = out + (((size_t)t * Hp + hp) * Wp + wp0) * 4;
    if (sizeof(T) == 2 && wp0 + 4 <= Wp && (Wp & 1) == 0) {
        // bf16: two pixels per 16-byte store (rows of an even Wp start 16-byte aligned)
#pragma unroll
        for (int j = 0; j < 4; j += 2) {
            V16 v;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const unsigned p = px[j + k];
                v.h[4 * k + 0] = from_f32<bf16_t>(lut[p & 255]);
                v.h[4 * k + 1] = from_f32<bf16_t>(lut[(p >> 8) & 255]);
                v.h[4 * k + 2] = from_f32<bf16_t>(lut[(p >> 16) & 255]);
                v.h[4 * k + 3] = from_f32<bf16_t>(0.f);
            }
            *(i32x4*)(o + 4 * j) = v.i;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (wp0 + j < Wp) store_px<T>(o + 4 * j, px[j], lut);
    }
}

// the same pixels as pitched NHWC [count][th][tw][ldd], channels 0..2 (what hdy_nchw_to_nhwc writes for a 3-channel image): plans whose first
// layer is not the 6x6/s2 stem.  One pixel per thread.
template <typename T>
__global__ __launch_bounds__(256) void slide_tiles_nhwc_kernel(const unsigned char* __restrict__ slide, long long pitch, int pb, int H, int W,
                                                               const int* __restrict__ origins, int first, T* __restrict__ out, int ldd, int th,
                                                               int tw, long long total, U8Table tab) {
    __shared__ float lut[256];
    lut[threadIdx.x] = tab.v[threadIdx.x];
    __syncthreads();
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const long long r = idx / tw;
    const int w = (int)(idx - r * tw);
    const int t = (int)(r / th), h = (int)(r - (long long)t * th);
    const long long y = (long long)origins[2 * (first + t) + 1] + h, x = (long long)origins[2 * (first + t)] + w;
    unsigned px = 0u;
    if (y >= 0 && y < H && x >= 0 && x < W) px = load1(slide + y * pitch + x * pb);
    T* o = out + (size_t)idx * ldd;
    o[0] = from_f32<T>(lut[px & 255]);
    o[1] = from_f32<T>(lut[(px >> 8) & 255]);
    o[2] = from_f32<T>(lut[(px >> 16) & 255]);
}

// counts[tile] = pixels of the tile's window (clipped to the slide) whose min(R, G, B) < background.  One workgroup per tile.
template <int PB>
__global__ __launch_bounds__(256) void slide_tissue_kernel(const unsigned char* __restrict__ slide, long long pitch, int H, int W,
                                                           const int* __restrict__ origins, int th, int tw, unsigned background,
                                                           int* __restrict__ counts) {
    __shared__ int part[4];
    const int t = blockIdx.x;
    const long long x0 = origins[2 * t], y0 = origins[2 * t + 1];
    const long long xs = x0 < 0 ? 0 : x0, ys = y0 < 0 ? 0 : y0;
    const long long xe = x0 + tw < W ? x0 + tw : W, ye = y0 + th < H ? y0 + th : H;
    int n = 0;
    if (xe > xs && ye > ys) {
        const int cols = (int)(xe - xs), rows = (int)(ye - ys), G = (cols + 3) >> 2;
        for (int item = threadIdx.x; item < rows * G; item += 256) {
            const int r = item / G, g = item - r * G;
            const unsigned char* p = slide + (ys + r) * pitch + (xs + 4 * g) * PB;
            if (4 * g + 4 <= cols) {
                unsigned px[4];
                load4<PB>(p, px);
#pragma unroll
                for (int j = 0; j < 4; ++j) n += is_tissue(px[j], background);
            } else {
                for (int j = 0; 4 * g + j < cols; ++j) n += is_tissue(load1(p + j * PB), background);
            }
        }
    }
    for (int m = 32; m >= 1; m >>= 1) n += __shfl_xor(n, m);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) counts[t] = part[0] + part[1] + part[2] + part[3];
}

constexpr int APPEND_MAX_B = 1024;

// One workgroup: prefix over n_keep, then every compacted row of the batch goes to out[cursor + row] with its tile's origin added to the box
// (one fp32 add per coordinate, as Detect.merge_outputs), then the cursor moves.  No atomics: same input, same bits.
__global__ __launch_bounds__(1024) void slide_append_kernel(const float* __restrict__ boxes, const float* __restrict__ scores,
                                                            const long long* __restrict__ labels, const int* __restrict__ n_keep, int B,
                                                            int in_rows, const int* __restrict__ origins, int first, float* __restrict__ out_boxes,
                                                            float* __restrict__ out_scores, long long* __restrict__ out_labels, int capacity,
                                                            int* __restrict__ cursor) {
    __shared__ int pre[APPEND_MAX_B + 1];
    const int base = cursor[0];
    for (int b = threadIdx.x; b < B; b += 1024) {
        const int n = n_keep[b];
        pre[b + 1] = n > 0 ? n : 0;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        pre[0] = 0;
        for (int b = 0; b < B; ++b) {
            s += pre[b + 1];
            pre[b + 1] = s;
        }
    }
    __syncthreads();
    const int total = pre[B];
    int room = capacity - base;
    room = room < 0 ? 0 : room;
    int fit = total < in_rows ? total : in_rows;
    fit = fit < room ? fit : room;
    for (int r = threadIdx.x; r < fit; r += 1024) {
        int lo = 0, hi = B - 1;                                  // the tile b with pre[b] <= r < pre[b + 1]
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (pre[mid + 1] <= r) lo = mid + 1;
            else hi = mid;
        }
        const float ox = (float)origins[2 * (first + lo)], oy = (float)origins[2 * (first + lo) + 1];
        const f32x4 bx = *(const f32x4*)(boxes + (size_t)r * 4);
        const size_t d = (size_t)base + r;
        f32x4 o = {__fadd_rn(bx[0], ox), __fadd_rn(bx[1], oy), __fadd_rn(bx[2], ox), __fadd_rn(bx[3], oy)};
        *(f32x4*)(out_boxes + d * 4) = o;
        out_scores[d] = scores[r];
        out_labels[d] = labels[r];
    }
    if (threadIdx.x == 0) {                                      // (every thread read cursor[0] before the first barrier)
        cursor[0] = base + fit;
        if (fit < total) cursor[1] = 1;
    }
}

}  // namespace

extern "C" {

int hdy_slide_tiles_u8(const unsigned char* slide, long long pitch_bytes, int pixel_bytes, int H, int W, const int* origins, int n_origins,
                       int first, int count, void* out, long long out_elems, int th, int tw, int pad, int ldd, int dtype, void* stream) {
    if (!slide_args_ok(slide, pitch_bytes, pixel_bytes, H, W, "slide_tiles_u8")) return HDY_EINVAL;
    HDY_ARG(origins && out, "slide_tiles_u8: null origin table or output");
    HDY_ARG(dtype == HDY_F32 || dtype == HDY_BF16, "slide_tiles_u8: dtype %d", dtype);
    HDY_ARG(th > 0 && tw > 0 && pad >= 0 && th <= (1 << 15) && tw <= (1 << 15) && pad <= 64, "slide_tiles_u8: tile %d x %d, pad %d", th, tw, pad);
    HDY_ARG(n_origins > 0 && first >= 0 && count > 0 && (long long)first + count <= n_origins,
            "slide_tiles_u8: rows [%d, %d + %d) lie beyond the origin table of %d rows", first, first, count, n_origins);
    hipStream_t st = (hipStream_t)stream;
    const U8Table& tab = u8_table();
    if (ldd == 0) {
        const long long Hp = th + 2 * pad, Wp = tw + 2 * pad;
        const long long want = (long long)count * Hp * Wp * 4;
        HDY_ARG(out_elems == want, "slide_tiles_u8: out holds %lld elements, count x (th + 2 pad) x (tw + 2 pad) x 4 = %lld expected", out_elems, want);
        HDY_ARG(((uintptr_t)out & 15) == 0, "slide_tiles_u8: out is not 16-byte aligned");
        const long long bpt = (Hp * ((Wp + 3) / 4) + 255) / 256;
        HDY_ARG(bpt * count < (1LL << 31), "slide_tiles_u8: grid too large");
        const dim3 grid((unsigned)(bpt * count));
#define HDY_SLIDE_STEM(T, PB)                                                                                                              \
    hipLaunchKernelGGL((slide_tiles_stem_kernel<T, PB>), grid, dim3(256), 0, st, slide, pitch_bytes, H, W, origins, first, (T*)out, th, tw, pad, \
                       (int)bpt, tab)
        if (dtype == HDY_BF16 && pixel_bytes == 3) HDY_SLIDE_STEM(bf16_t, 3);
        else if (dtype == HDY_BF16) HDY_SLIDE_STEM(bf16_t, 4);
        else if (pixel_bytes == 3) HDY_SLIDE_STEM(float, 3);
        else HDY_SLIDE_STEM(float, 4);
#undef HDY_SLIDE_STEM
        hdy_note_dispatch("slide_tiles_u8_stem");
    } else {
        HDY_ARG(pad == 0 && ldd >= 3, "slide_tiles_u8: pitched NHWC output takes pad 0 and a pixel pitch >= 3 (pad %d, pitch %d)", pad, ldd);
        const long long total = (long long)count * th * tw;
        HDY_ARG(out_elems == total * ldd, "slide_tiles_u8: out holds %lld elements, count x th x tw x pitch = %lld expected", out_elems, total * ldd);
        HDY_ARG((total + 255) / 256 < (1LL << 31), "slide_tiles_u8: grid too large");
        const dim3 grid((unsigned)((total + 255) / 256));
        if (dtype == HDY_BF16)
            hipLaunchKernelGGL(slide_tiles_nhwc_kernel<bf16_t>, grid, dim3(256), 0, st, slide, pitch_bytes, pixel_bytes, H, W, origins, first,
                               (bf16_t*)out, ldd, th, tw, total, tab);
        else
            hipLaunchKernelGGL(slide_tiles_nhwc_kernel<float>, grid, dim3(256), 0, st, slide, pitch_bytes, pixel_bytes, H, W, origins, first,
                               (float*)out, ldd, th, tw, total, tab);
        hdy_note_dispatch("slide_tiles_u8_nhwc");
    }
    HDY_LAUNCH_CHECK("slide_tiles_u8");
    return HDY_OK;
}

int hdy_slide_append(const float* boxes, const float* scores, const long long* labels, const int* n_keep, int B, int in_rows, const int* origins,
                     int n_origins, int first, float* out_boxes, float* out_scores, long long* out_labels, int capacity, int* cursor, void* stream) {
    HDY_ARG(boxes && scores && labels && n_keep && origins && out_boxes && out_scores && out_labels && cursor, "slide_append: null pointer");
    HDY_ARG(B > 0 && B <= APPEND_MAX_B, "slide_append: batch of %d tiles (1 .. %d)", B, APPEND_MAX_B);
    HDY_ARG(in_rows > 0, "slide_append: input arrays of %d rows", in_rows);
    HDY_ARG(n_origins > 0 && first >= 0 && (long long)first + B <= n_origins,
            "slide_append: rows [%d, %d + %d) lie beyond the origin table of %d rows", first, first, B, n_origins);
    HDY_ARG(capacity > 0, "slide_append: capacity of %d rows", capacity);
    HDY_ARG((((uintptr_t)boxes | (uintptr_t)out_boxes) & 15) == 0, "slide_append: box arrays are not 16-byte aligned");
    hipLaunchKernelGGL(slide_append_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, boxes, scores, labels, n_keep, B, in_rows, origins, first,
                       out_boxes, out_scores, out_labels, capacity, cursor);
    HDY_LAUNCH_CHECK("slide_append");
    return HDY_OK;
}

int hdy_slide_tissue_u8(const unsigned char* slide, long long pitch_bytes, int pixel_bytes, int H, int W, const int* origins, int n_origins, int th,
                        int tw, int background, int* counts, int n_counts, void* stream) {
    if (!slide_args_ok(slide, pitch_bytes, pixel_bytes, H, W, "slide_tissue_u8")) return HDY_EINVAL;
    HDY_ARG(origins && counts, "slide_tissue_u8: null origin table or counts");
    HDY_ARG(n_origins > 0 && n_counts == n_origins, "slide_tissue_u8: %d counts for an origin table of %d rows", n_counts, n_origins);
    HDY_ARG(th > 0 && tw > 0 && th <= (1 << 15) && tw <= (1 << 15), "slide_tissue_u8: tile %d x %d", th, tw);
    HDY_ARG(background >= 0 && background <= 256, "slide_tissue_u8: background %d (0 .. 256)", background);
    if (pixel_bytes == 3)
        hipLaunchKernelGGL(slide_tissue_kernel<3>, dim3(n_origins), dim3(256), 0, (hipStream_t)stream, slide, pitch_bytes, H, W, origins, th, tw,
                           (unsigned)background, counts);
    else
        hipLaunchKernelGGL(slide_tissue_kernel<4>, dim3(n_origins), dim3(256), 0, (hipStream_t)stream, slide, pitch_bytes, H, W, origins, th, tw,
                           (unsigned)background, counts);
    hdy_note_dispatch("slide_tissue_u8");
    HDY_LAUNCH_CHECK("slide_tissue_u8");
    return HDY_OK;
}

}  // extern "C"
