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
// Box kernel (augment_common.h, shared with csrc/augment_masks.hip): one workgroup of 1024 threads.  The candidates (image, cell in (r, c)
// order, source order) are walked 1024 at a time; each chunk's keep flags are prefix-summed, so the compact order is the candidate order and
// repeats give the same bits.  No atomics.
#include <hip/hip_runtime.h>

#include "augment_common.h"

namespace {

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
    int qx, qy;
    if (!canvas_to_q(cp, u, v, &qx, &qy)) return cvp;                            // NaN and far away: border
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
    hipLaunchKernelGGL(augment_boxes_kernel<false>, dim3(1), dim3(1024), 0, (hipStream_t)stream, bank_boxes, bank_labels, offsets, n, M,
                       (const unsigned*)cells, crop, B, patch, k, img_size, out_boxes, out_labels, out_img, cap, counts, overflow, MaskRows{});
    hdy_note_dispatch("augment_boxes");
    HDY_LAUNCH_CHECK("augment_boxes");
    return HDY_OK;
}

}  // extern "C"
