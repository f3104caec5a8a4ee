// Training augmentation from an 8-bit tile bank that stays on the device: one launch writes the augmented NCHW batch, one writes the transformed
// and compacted targets.  Reference call sites: TorchDataset.__getitem__'s training branch (metayolo/datasets.py: k x k mosaic of train_proc'ed
// tiles, random crop, small-object filter, target_to_tensors) with train_proc = random_hsv -> random_projective -> random_flip
// (metayolo/engines/image_utils.py random_hsv / random_transform_pars / estimate_matrix / warp_coords / Mask, augmentations.py box_candidates).
// The parameters are drawn and the matrices composed on the host (hd_yolo_amd/augment.py); the kernels apply them.  include/hdyolo.h states every
// formula below; tests/augment_ref.py restates them on the CPU, and the two must agree bit for bit.
//
// Image kernel: a gather, one workgroup per band of AUG_ROWS output rows of one image, each thread two neighbouring pixels of a row so that a
// wave writes 256 contiguous bytes per colour plane (bf16).  The cells a band can touch (two mosaic rows x k columns) sit in LDS with their
// matrices and HSV tables.  No MFMA, no LDS-DMA.  Source bytes are read as aligned dwords (at most 3 bytes beside a pixel, never another page).
// Workgroups of one image get neighbouring logical ids on one XCD (xcd_remap), so the four texel reads of neighbouring pixels meet in its L2.
//
// Box kernel: one workgroup of 1024 threads.  The candidates (image, cell in (r, c) order, source order) are walked 1024 at a time; each chunk's
// keep flags are prefix-summed, so the compact order is the candidate order and repeats give the same bits.  No atomics.
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

// v / 255 correctly rounded to fp32 (the table of slide.hip: made on the host with IEEE division, handed to the kernel by value)
struct U8Table {
    float v[256];
};

const U8Table& u8_table() {
    static const U8Table tab = [] {
        U8Table t;
        for (int i = 0; i < 256; ++i) {
            volatile float num = (float)i, den = 255.0f;
            t.v[i] = num / den;
        }
        return t;
    }();
    return tab;
}

// the PB-byte pixel at p as r | g << 8 | b << 16, from the aligned dword(s) that hold its three colour bytes
__device__ __forceinline__ unsigned load_px(const unsigned char* p) {
    const unsigned mis = (unsigned)((uintptr_t)p & 3);
    const unsigned* q = (const unsigned*)(p - mis);
    const unsigned d0 = q[0];
    const unsigned d1 = mis >= 2 ? q[1] : 0u;                  // the second dword only when it holds one of the three bytes
    return __funnelshift_r(d0, d1, mis * 8) & 0xFFFFFFu;
}

// 8-bit RGB -> HSV (H in 0..179) -> the cell's three tables -> RGB, all in integers (include/hdyolo.h, "HSV round trip")
__device__ __forceinline__ unsigned hsv_round_trip(unsigned px, const unsigned char* lut) {
    const int r = px & 255, g = (px >> 8) & 255, b = (px >> 16) & 255;
    const int V = max(r, max(g, b)), mn = min(r, min(g, b)), d = V - mn;
    const int S = V ? (255 * d + (V >> 1)) / V : 0;
    int H = 0;
    if (d) {
        int num, off;
        if (V == r) { num = g - b; off = 0; }
        else if (V == g) { num = b - r; off = 60; }
        else { num = r - g; off = 120; }
        H = off + (60 * (num + d) + d) / (2 * d) - 30;         // off + floor(30 num / d + 1/2)
        if (H < 0) H += 180;
    }
    int Hn = lut[H];
    const int Sn = lut[256 + S], Vn = lut[512 + V];
    if (Hn >= 180) Hn -= 180;                                  // a table made by (x r) % 180 never gets here; any table is safe
    const int sec = Hn / 30, f = Hn - 30 * sec;
    const int p = (Vn * (255 - Sn) + 127) / 255;
    const int q = (Vn * (7650 - Sn * f) + 3825) / 7650;
    const int t = (Vn * (7650 - Sn * (30 - f)) + 3825) / 7650;
    int R, G, B;
    switch (sec) {
        case 0: R = Vn; G = t; B = p; break;
        case 1: R = q; G = Vn; B = p; break;
        case 2: R = p; G = Vn; B = t; break;
        case 3: R = p; G = q; B = Vn; break;
        case 4: R = t; G = p; B = Vn; break;
        default: R = Vn; G = p; B = q; break;
    }
    return (unsigned)R | ((unsigned)G << 8) | ((unsigned)B << 16);
}

struct BankView {
    const unsigned char* base;
    long long tile_stride, pitch;
    int n, H, W;
};

// one output pixel of the mosaic at (X, Y) (already offset by the crop): packed r | g << 8 | b << 16 bytes
template <int PB>
__device__ __forceinline__ unsigned augment_pixel(const BankView& bk, const unsigned* lc, int X, int Y, int r, int rr, int P, int k, unsigned cvp) {
    const int c = X / P;
    const unsigned* cp = lc + (rr * k + c) * CELL_WORDS;
    const unsigned flags = cp[W_FLAGS];
    int u = X - c * P, v = Y - r * P;
    if (flags & F_TRANSPOSE) { const int t = u; u = v; v = t; }
    if (flags & F_VFLIP) v = P - 1 - v;
    if (flags & F_HFLIP) u = P - 1 - u;
    const float fu = (float)u, fv = (float)v;
    const float* m = (const float*)cp + W_INV;
    float sx = __fadd_rn(__fadd_rn(__fmul_rn(m[0], fu), __fmul_rn(m[1], fv)), m[2]);
    float sy = __fadd_rn(__fadd_rn(__fmul_rn(m[3], fu), __fmul_rn(m[4], fv)), m[5]);
    if (flags & F_PERSP) {
        const float sw = __fadd_rn(__fadd_rn(__fmul_rn(m[6], fu), __fmul_rn(m[7], fv)), m[8]);
        sx = __fdiv_rn(sx, sw);
        sy = __fdiv_rn(sy, sw);
    }
    const float tx = __fmul_rn(sx, 32.0f), ty = __fmul_rn(sy, 32.0f);
    const float LIM = 16777216.0f;
    if (!(tx >= -LIM && tx <= LIM && ty >= -LIM && ty <= LIM)) return cvp;       // NaN and far away: border
    const int qx = __float2int_rn(tx), qy = __float2int_rn(ty);
    const int x0 = qx >> 5, y0 = qy >> 5, fx = qx & 31, fy = qy & 31;
    const int src = (int)cp[W_SRC];
    if (src < 0 || src >= bk.n || x0 < -1 || x0 >= bk.W || y0 < -1 || y0 >= bk.H) return cvp;
    const unsigned char* tile = bk.base + (long long)src * bk.tile_stride;
    const unsigned char* lut = (const unsigned char*)(cp + W_LUT);
    unsigned t[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int x = x0 + (j & 1), y = y0 + (j >> 1);
        t[j] = cvp;
        if (x >= 0 && x < bk.W && y >= 0 && y < bk.H) {
            t[j] = load_px(tile + (long long)y * bk.pitch + (long long)x * PB);
            if (flags & F_HSV) t[j] = hsv_round_trip(t[j], lut);
        }
    }
    const unsigned w00 = (32 - fx) * (32 - fy), w01 = fx * (32 - fy), w10 = (32 - fx) * fy, w11 = fx * fy;
    unsigned res = 0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const unsigned sh = 8 * ch;
        const unsigned a = ((t[0] >> sh) & 255) * w00 + ((t[1] >> sh) & 255) * w01 + ((t[2] >> sh) & 255) * w10 + ((t[3] >> sh) & 255) * w11;
        res |= ((a + 512) >> 10) << sh;
    }
    return res;
}

template <typename T, int PB>
__global__ __launch_bounds__(256) void augment_tiles_kernel(BankView bk, const unsigned* __restrict__ cells, const int* __restrict__ crop,
                                                            T* __restrict__ out, int P, int k, int S, unsigned cval, int nbands, U8Table tab) {
    __shared__ unsigned lc[2 * AUG_KMAX * CELL_WORDS];
    __shared__ float lut[256];
    lut[threadIdx.x] = tab.v[threadIdx.x];
    const int wi = xcd_remap((int)blockIdx.x, (int)gridDim.x);
    const int b = wi / nbands, oy0 = (wi - b * nbands) * AUG_ROWS;
    const int cx = crop[2 * b], cy = crop[2 * b + 1];
    const bool crop_ok = cx >= 0 && cy >= 0 && cx <= k * P - S && cy <= k * P - S;   // any other offset: the image is the border value
    const int r0 = crop_ok ? (cy + oy0) / P : 0;
    if (crop_ok) {
        for (int i = threadIdx.x; i < 2 * k * CELL_WORDS; i += 256) {
            const int slot = i / CELL_WORDS, word = i - slot * CELL_WORDS;
            const int rr = slot / k, c = slot - rr * k, r = r0 + rr;
            lc[i] = r < k ? cells[((size_t)(b * k + r) * k + c) * CELL_WORDS + word] : 0u;
        }
    }
    __syncthreads();
    const unsigned cvp = cval * 0x010101u;
    const int npairs = (S + 1) >> 1;
    const int rows = min(AUG_ROWS, S - oy0);
    const size_t plane = (size_t)S * S;
    for (int item = threadIdx.x; item < rows * npairs; item += 256) {
        const int j = item / npairs, x = 2 * (item - j * npairs), oy = oy0 + j;
        unsigned px[2] = {cvp, cvp};
        if (crop_ok) {
            const int Y = cy + oy, r = Y / P;
            px[0] = augment_pixel<PB>(bk, lc, cx + x, Y, r, r - r0, P, k, cvp);
            if (x + 1 < S) px[1] = augment_pixel<PB>(bk, lc, cx + x + 1, Y, r, r - r0, P, k, cvp);
        }
        T* o = out + ((size_t)b * 3 * S + oy) * S + x;
        if ((S & 1) == 0) {                                    // rows start on an even element: both pixels of a plane in one store
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const T v0 = from_f32<T>(lut[(px[0] >> (8 * ch)) & 255]), v1 = from_f32<T>(lut[(px[1] >> (8 * ch)) & 255]);
                T pair[2] = {v0, v1};
                if (sizeof(T) == 2) *(unsigned*)(o + ch * plane) = *(const unsigned*)pair;
                else *(unsigned long long*)(o + ch * plane) = *(const unsigned long long*)pair;
            }
        } else {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                o[ch * plane] = from_f32<T>(lut[(px[0] >> (8 * ch)) & 255]);
                if (x + 1 < S) o[ch * plane + 1] = from_f32<T>(lut[(px[1] >> (8 * ch)) & 255]);
            }
        }
    }
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

// one source box through a cell's forward matrix, candidate test, flips, mosaic and crop offsets, the two filters, normalisation
// (include/hdyolo.h, "Targets"); false: dropped
__device__ __forceinline__ bool augment_box(const float* bx, const unsigned* cp, int r, int c, int P, int S, int cx, int cy, float* o) {
    const float* F = (const float*)cp + W_FWD;
    const float sc = ((const float*)cp)[W_SCALE];
    const unsigned flags = cp[W_FLAGS];
    const float fP = (float)P, fS = (float)S;
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
    const float eps = 1e-16f;
    const float w1 = __fsub_rn(__fmul_rn(bx[2], sc), __fmul_rn(bx[0], sc)), h1 = __fsub_rn(__fmul_rn(bx[3], sc), __fmul_rn(bx[1], sc));
    const float w2 = __fsub_rn(x2, x1), h2 = __fsub_rn(y2, y1);
    const float ar = fmaxf(__fdiv_rn(w2, __fadd_rn(h2, eps)), __fdiv_rn(h2, __fadd_rn(w2, eps)));
    const float ratio = __fdiv_rn(__fmul_rn(w2, h2), __fadd_rn(__fmul_rn(w1, h1), eps));
    if (!(w2 > 2.0f && h2 > 2.0f && ratio > 0.1f && ar < 100.0f)) return false;
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

__global__ __launch_bounds__(1024) void augment_boxes_kernel(const float* __restrict__ bank_boxes, const long long* __restrict__ bank_labels,
                                                             const long long* __restrict__ offsets, int n, int M, const unsigned* __restrict__ cells,
                                                             const int* __restrict__ crop, int B, int P, int k, int S, float* __restrict__ out_boxes,
                                                             long long* __restrict__ out_labels, float* __restrict__ out_img, int cap,
                                                             int* __restrict__ counts, int* __restrict__ overflow) {
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
        int keep = 0, ci = 0, b = 0;
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
            row = offsets[(int)cp[W_SRC]] + (t - cstart[ci]);
            const f32x4 v = *(const f32x4*)(bank_boxes + row * 4);
            const float bx[4] = {v[0], v[1], v[2], v[3]};
            keep = augment_box(bx, cp, r, c, P, S, crop[2 * b], crop[2 * b + 1], o) ? 1 : 0;
        }
        int total;
        const int ex = block_scan_1024(keep, wsum, &total);
        if (t < T && t == cstart[ci]) cpos[ci] = base + ex;
        if (keep && base + ex < cap) {
            const size_t d = (size_t)(base + ex);
            f32x4 w = {o[0], o[1], o[2], o[3]};
            *(f32x4*)(out_boxes + d * 4) = w;
            out_labels[d] = bank_labels[row];
            out_img[d] = (float)b;
        }
        base += total;
    }
    __syncthreads();
    if (tid == 0) {
        cpos[ncell] = base;
        for (int ci = ncell - 1; ci >= 0; --ci)
            if (cstart[ci + 1] == cstart[ci]) cpos[ci] = cpos[ci + 1];       // a cell without candidates starts where the next one does
        overflow[0] = base > cap ? 1 : 0;
    }
    __syncthreads();
    for (int b = tid; b < B; b += 1024) counts[b] = cpos[(b + 1) * k2] - cpos[b * k2];
}

bool mosaic_args_ok(const void* cells, int n_cells, const void* crop, int B, int patch, int k, int img_size, const char* who) {
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

extern "C" {

int hdy_augment_tiles_u8(const unsigned char* bank, long long tile_stride_bytes, long long pitch_bytes, int pixel_bytes, int n, int H, int W,
                         const void* cells, int n_cells, const int* crop, int B, int patch, int k, int img_size, int cval, void* out,
                         long long out_elems, int dtype, void* stream) {
    HDY_ARG(bank && out, "augment_tiles_u8: null bank or output");
    HDY_ARG(pixel_bytes == 3 || pixel_bytes == 4, "augment_tiles_u8: pixel_bytes is %d, 3 (RGB) or 4 (RGBA) expected", pixel_bytes);
    HDY_ARG(n > 0 && H > 0 && W > 0 && H <= (1 << 15) && W <= (1 << 15), "augment_tiles_u8: bank of %d tiles of %d x %d pixels", n, H, W);
    HDY_ARG(pitch_bytes >= (long long)W * pixel_bytes, "augment_tiles_u8: row pitch of %lld bytes is below W * pixel_bytes = %lld", pitch_bytes,
            (long long)W * pixel_bytes);
    HDY_ARG(tile_stride_bytes >= (long long)(H - 1) * pitch_bytes + (long long)W * pixel_bytes,
            "augment_tiles_u8: tile stride of %lld bytes is below a tile's extent", tile_stride_bytes);
    HDY_ARG(dtype == HDY_F32 || dtype == HDY_BF16, "augment_tiles_u8: dtype %d", dtype);
    HDY_ARG(cval >= 0 && cval <= 255, "augment_tiles_u8: border value %d (0 .. 255)", cval);
    if (!mosaic_args_ok(cells, n_cells, crop, B, patch, k, img_size, "augment_tiles_u8")) return HDY_EINVAL;
    const long long want = (long long)B * 3 * img_size * img_size;
    HDY_ARG(out_elems == want, "augment_tiles_u8: out holds %lld elements, B x 3 x img_size x img_size = %lld expected", out_elems, want);
    HDY_ARG(((uintptr_t)out & 15) == 0, "augment_tiles_u8: out is not 16-byte aligned");
    const int nbands = (img_size + AUG_ROWS - 1) / AUG_ROWS;
    HDY_ARG((long long)B * nbands < (1LL << 31), "augment_tiles_u8: grid too large");
    const dim3 grid((unsigned)(B * nbands));
    const BankView bk{bank, tile_stride_bytes, pitch_bytes, n, H, W};
    const U8Table& tab = u8_table();
#define HDY_AUG_TILES(T, PB)                                                                                                               \
    hipLaunchKernelGGL((augment_tiles_kernel<T, PB>), grid, dim3(256), 0, (hipStream_t)stream, bk, (const unsigned*)cells, crop, (T*)out, patch, k, \
                       img_size, (unsigned)cval, nbands, tab)
    if (dtype == HDY_BF16 && pixel_bytes == 3) HDY_AUG_TILES(bf16_t, 3);
    else if (dtype == HDY_BF16) HDY_AUG_TILES(bf16_t, 4);
    else if (pixel_bytes == 3) HDY_AUG_TILES(float, 3);
    else HDY_AUG_TILES(float, 4);
#undef HDY_AUG_TILES
    hdy_note_dispatch("augment_tiles_u8");
    HDY_LAUNCH_CHECK("augment_tiles_u8");
    return HDY_OK;
}

int hdy_augment_boxes(const float* bank_boxes, const long long* bank_labels, const long long* offsets, int n, int M, const void* cells, int n_cells,
                      const int* crop, int B, int patch, int k, int img_size, float* out_boxes, long long* out_labels, float* out_img, int cap,
                      int* counts, int n_counts, int* overflow, void* stream) {
    HDY_ARG(bank_boxes && bank_labels && offsets && out_boxes && out_labels && out_img && counts && overflow, "augment_boxes: null pointer");
    HDY_ARG(n > 0 && M >= 0, "augment_boxes: bank of %d tiles with %d boxes", n, M);
    if (!mosaic_args_ok(cells, n_cells, crop, B, patch, k, img_size, "augment_boxes")) return HDY_EINVAL;
    HDY_ARG(n_cells <= BOX_MAX_CELLS, "augment_boxes: %d cells in one call (at most %d)", n_cells, BOX_MAX_CELLS);
    HDY_ARG(cap > 0, "augment_boxes: capacity of %d rows", cap);
    HDY_ARG(n_counts == B, "augment_boxes: %d counts for %d images", n_counts, B);
    HDY_ARG((((uintptr_t)bank_boxes | (uintptr_t)out_boxes) & 15) == 0, "augment_boxes: box arrays are not 16-byte aligned");
    hipLaunchKernelGGL(augment_boxes_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, bank_boxes, bank_labels, offsets, n, M,
                       (const unsigned*)cells, crop, B, patch, k, img_size, out_boxes, out_labels, out_img, cap, counts, overflow);
    hdy_note_dispatch("augment_boxes");
    HDY_LAUNCH_CHECK("augment_boxes");
    return HDY_OK;
}

}  // extern "C"
