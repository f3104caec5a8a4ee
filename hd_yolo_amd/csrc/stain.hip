// Stain estimation counts and recolouring of an 8-bit slide (include/hdyolo_stain.h): the ten optical-density moments, the histogram of
// angles in the plane of the two leading eigenvectors, the per-stain level histograms, and the recolouring pass.  Streams over 3 or 4 bytes
// per pixel with a few table reads and integer operations per pixel; no MFMA, no LDS-DMA, no floating point, no atomics on global memory.
//
// The arithmetic is stated in include/hdyolo_stain.h and restated in tests/stain_ref.py.
//
// The three counting passes share one walk: the visited pixels of a row are cut into groups of four (one aligned multi-dword load where
// step = 1 and the group is whole, byte loads at the row's tail and for step > 1), the groups of the window are numbered row by row, and a
// workgroup takes one contiguous run of them, 512 at a time.  A lane finds (row, group) by one 64-bit division and then steps by a
// precomputed (rows, groups) increment.  Every workgroup leaves one slab of int64 cells in the workspace and reduce_kernel adds the slabs
// in a fixed order: same input, same bits, and no zeroing launch.
//
// moments_kernel: ten 32-bit sums per lane over at most 256 pixels (4095^2 * 256 < 2^32), then into 64 bits; wave shuffles, one LDS row per
// wave, one slab row per workgroup.
// hist_kernel<ANGLES>: on real tissue most pixels fall into a few dozen bins, so one LDS histogram per workgroup would serialise on LDS
// atomics.  Two measures: a lane merges equal bins among its four neighbouring pixels before it adds, and the workgroup keeps `copies`
// sub-histograms (as many as fit beside the table in 48 KB, at most 16: 10 at A = 1024, 5 at B = 1024, 16 up to 670 cells), lane t adding
// to copy t % copies so that neighbouring lanes, whose pixels are alike, do not meet.  Rows have an odd number of words, which spreads equal
// bins of different copies over the banks.  The copies are added up when the slab row is written.
// apply_kernel: both tables in LDS (9 KB + T bytes), four pixels per lane, 12- or 16-byte stores where the destination is aligned.
#include "slide_common.h"
#include "hdyolo_stain.h"

namespace {

constexpr int THREADS = 512;                     // the counting passes
constexpr int APPLY_THREADS = 256;
constexpr int MAX_BLOCKS = HDY_STAIN_MAX_BLOCKS;
constexpr int APPLY_MAX_BLOCKS = 1 << 16;
constexpr int ITEMS_PER_LANE = 8;                // groups of four pixels a lane sees at least, before a second workgroup is worth its slab
constexpr int HIST_LDS_BYTES = 48 * 1024;
constexpr int HIST_MAX_BLOCKS = 768;             // three workgroups of 48 KB fit a CU's LDS, 256 CUs: every workgroup resident, one round
static_assert(HIST_MAX_BLOCKS <= MAX_BLOCKS, "the workspace is sized by HDY_STAIN_MAX_BLOCKS");
constexpr int MAX_COPIES = 16;
constexpr int ANGLE_SHIFT = HDY_STAIN_ANGLE_SHIFT, SHIFT = HDY_STAIN_SHIFT;

struct Win {
    const unsigned char* slide;
    long long pitch;
    int x0, y0, nx, ny, step;                    // nx x ny visited pixels, `step` apart
    unsigned background;
    int G;                                       // groups of four per row
    long long items, chunk;                      // G * ny groups, `chunk` of them per workgroup
    int dr, dg;                                  // one stride of the workgroup's threads, in (rows, groups)
};

struct Walk {
    long long item, last;
    int r, g;
};

__device__ __forceinline__ Walk walk_begin(const Win& a) {
    Walk w;
    const long long first = (long long)blockIdx.x * a.chunk;
    w.last = first + a.chunk < a.items ? first + a.chunk : a.items;
    w.item = first + threadIdx.x;
    w.r = w.g = 0;
    if (w.item < w.last) {
        const long long r = w.item / a.G;
        w.r = (int)r;
        w.g = (int)(w.item - r * a.G);
    }
    return w;
}

__device__ __forceinline__ void walk_next(const Win& a, Walk& w) {
    w.item += blockDim.x;
    w.g += a.dg;
    w.r += a.dr;
    if (w.g >= a.G) {
        w.g -= a.G;
        ++w.r;
    }
}

// the visited pixels 4 g .. 4 g + 3 of visited row r (those below nx): their number, and the pixels as r | g << 8 | b << 16
template <int PB>
__device__ __forceinline__ int fetch(const Win& a, int r, int g, unsigned* px) {
    const unsigned char* row = a.slide + ((long long)a.y0 + (long long)r * a.step) * a.pitch;
    const int i0 = 4 * g;
    if (a.step == 1 && i0 + 4 <= a.nx) {
        load4<PB>(row + ((long long)a.x0 + i0) * PB, px);
        return 4;
    }
    const int c = a.nx - i0 < 4 ? a.nx - i0 : 4;
    for (int j = 0; j < c; ++j) px[j] = load1(row + ((long long)a.x0 + (long long)(i0 + j) * a.step) * PB);
    return c;
}

template <int PB>
__global__ __launch_bounds__(THREADS) void moments_kernel(const Win a, const int* __restrict__ od, long long* __restrict__ slab) {
    constexpr int WAVES = THREADS / 64;
    __shared__ int od_s[256];
    __shared__ unsigned long long part[WAVES][10];
    if (threadIdx.x < 256) od_s[threadIdx.x] = od[threadIdx.x];
    __syncthreads();
    unsigned long long tot[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) tot[k] = 0;
    Walk w = walk_begin(a);
    while (w.item < w.last) {
        unsigned acc[10];
#pragma unroll
        for (int k = 0; k < 10; ++k) acc[k] = 0;
        for (int it = 0; it < 64 && w.item < w.last; ++it, walk_next(a, w)) {       // 256 pixels: the 32-bit sums cannot wrap
            unsigned px[4];
            const int c = fetch<PB>(a, w.r, w.g, px);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j >= c || !is_tissue(px[j], a.background)) continue;
                const unsigned qr = (unsigned)od_s[px[j] & 255], qg = (unsigned)od_s[(px[j] >> 8) & 255], qb = (unsigned)od_s[(px[j] >> 16) & 255];
                acc[0] += 1; acc[1] += qr; acc[2] += qg; acc[3] += qb;
                acc[4] += qr * qr; acc[5] += qr * qg; acc[6] += qr * qb;
                acc[7] += qg * qg; acc[8] += qg * qb; acc[9] += qb * qb;
            }
        }
#pragma unroll
        for (int k = 0; k < 10; ++k) tot[k] += acc[k];
    }
#pragma unroll
    for (int k = 0; k < 10; ++k)
        for (int m = 32; m >= 1; m >>= 1) tot[k] += __shfl_xor(tot[k], m);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 10; ++k) part[threadIdx.x >> 6][k] = tot[k];
    }
    __syncthreads();
    if (threadIdx.x < 10) {
        unsigned long long s = 0;
        for (int v = 0; v < WAVES; ++v) s += part[v][threadIdx.x];
        slab[(long long)blockIdx.x * 10 + threadIdx.x] = (long long)s;
    }
}

__device__ __forceinline__ int table_sum(const int* t, unsigned px) {
    return (int)((unsigned)t[px & 255] + (unsigned)t[256 + ((px >> 8) & 255)] + (unsigned)t[512 + ((px >> 16) & 255)]);      // modulo 2^32
}

__device__ __forceinline__ int clamp_index(int v, int n) { return v < 0 ? 0 : v > n - 1 ? n - 1 : v; }

// one histogram's run of equal bins among a lane's pixels: add when the bin changes
struct Run {
    int bin;
    unsigned n;
    __device__ __forceinline__ void put(unsigned* h, int b) {
        if (b == bin) {
            ++n;
        } else {
            if (n) atomicAdd(&h[bin], n);
            bin = b;
            n = 1;
        }
    }
    __device__ __forceinline__ void flush(unsigned* h) {
        if (n) atomicAdd(&h[bin], n);
        n = 0;
    }
};

// ANGLES: cells = A + 1, cell A counts the skipped pixels.  Levels: cells = 2 * bins, stain s in cells [s * bins, (s + 1) * bins).
template <int PB, bool ANGLES>
__global__ __launch_bounds__(THREADS) void hist_kernel(const Win a, const int* __restrict__ lut, int bins, int cells, int copies,
                                                       long long* __restrict__ slab) {
    extern __shared__ int lds[];
    int* lut_s = lds;                                        // [2][3][256]
    unsigned* hist_s = (unsigned*)(lds + 1536);              // [copies][stride]
    const int stride = cells | 1;
    for (int k = threadIdx.x; k < 1536; k += THREADS) lut_s[k] = lut[k];
    for (int k = threadIdx.x; k < copies * stride; k += THREADS) hist_s[k] = 0;
    __syncthreads();
    unsigned* mine = hist_s + (threadIdx.x % copies) * stride;
    for (Walk w = walk_begin(a); w.item < w.last; walk_next(a, w)) {
        unsigned px[4];
        const int c = fetch<PB>(a, w.r, w.g, px);
        Run r0 = {0, 0}, r1 = {0, 0};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j >= c || !is_tissue(px[j], a.background)) continue;
            const int t0 = table_sum(lut_s, px[j]), t1 = table_sum(lut_s + 768, px[j]);
            if (ANGLES) {
                const int p0 = t0 >> ANGLE_SHIFT, p1 = t1 >> ANGLE_SHIFT;
                int bin = bins;                              // skipped
                if (p0 > 0) {
                    const unsigned s = (unsigned)p0 + (unsigned)(p1 < 0 ? -p1 : p1);
                    const unsigned q = (unsigned)bins * (s + (unsigned)p1) / (2u * s);      // exact unsigned quotient
                    bin = q < (unsigned)bins ? (int)q : bins - 1;                           // (only a table beyond the bound gets here clamped)
                }
                r0.put(mine, bin);
            } else {
                r0.put(mine, clamp_index(t0 >> SHIFT, bins));
                r1.put(mine, bins + clamp_index(t1 >> SHIFT, bins));
            }
        }
        r0.flush(mine);
        if (!ANGLES) r1.flush(mine);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < cells; k += THREADS) {
        unsigned long long s = 0;
        for (int v = 0; v < copies; ++v) s += hist_s[v * stride + k];
        slab[(long long)blockIdx.x * cells + k] = (long long)s;
    }
}

// out[cell] = the sum over the slab rows, in row order per partial and partial order after: cells [0, n0) go to out0, the rest to out1
__global__ __launch_bounds__(1024) void reduce_kernel(const long long* __restrict__ slab, int rows, int cells, long long* __restrict__ out0, int n0,
                                                      long long* __restrict__ out1) {
    __shared__ long long part[16][64];
    const int c = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const int cell = blockIdx.x * 64 + c;
    long long s = 0;
    if (cell < cells)
        for (int b = grp; b < rows; b += 16) s += slab[(long long)b * cells + cell];
    part[grp][c] = s;
    __syncthreads();
    if (grp == 0 && cell < cells) {
        for (int v = 1; v < 16; ++v) s += part[v][c];
        if (cell < n0) out0[cell] = s;
        else out1[cell - n0] = s;
    }
}

struct ApplyArgs {
    Win win;                                     // step 1, nx x ny = the window
    unsigned char* dst;
    long long dst_pitch;
    const int* lut;
    const unsigned char* tone;
    int T;
};

__device__ __forceinline__ unsigned recolour(const int* lut_s, const unsigned char* tone_s, int T, unsigned px) {
    const unsigned r = tone_s[clamp_index(table_sum(lut_s, px) >> SHIFT, T)];
    const unsigned g = tone_s[clamp_index(table_sum(lut_s + 768, px) >> SHIFT, T)];
    const unsigned b = tone_s[clamp_index(table_sum(lut_s + 1536, px) >> SHIFT, T)];
    return r | (g << 8) | (b << 16);
}

template <int SPB, int DPB>
__global__ __launch_bounds__(APPLY_THREADS) void apply_kernel(const ApplyArgs a) {
    __shared__ int lut_s[2304];
    __shared__ unsigned char tone_s[HDY_STAIN_MAX_TONE];
    for (int k = threadIdx.x; k < 2304; k += APPLY_THREADS) lut_s[k] = a.lut[k];
    for (int k = threadIdx.x; k < a.T; k += APPLY_THREADS) tone_s[k] = a.tone[k];
    __syncthreads();
    const Win& win = a.win;
    for (Walk w = walk_begin(win); w.item < w.last; walk_next(win, w)) {
        const long long y = (long long)win.y0 + w.r, x = (long long)win.x0 + 4 * w.g;
        const unsigned char* p = win.slide + y * win.pitch + x * SPB;
        unsigned char* q = a.dst + y * a.dst_pitch + x * DPB;
        const int c = win.nx - 4 * w.g < 4 ? win.nx - 4 * w.g : 4;
        unsigned in[4], o[4];                    // r | g << 8 | b << 16 | alpha << 24
        if (c == 4) {
            if (SPB == 4) load4_raw<4>(p, in);
            else load4<3>(p, in);
        } else {
            for (int j = 0; j < c; ++j) in[j] = load1(p + j * SPB) | (SPB == 4 ? (unsigned)p[j * SPB + 3] << 24 : 0u);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < c) o[j] = recolour(lut_s, tone_s, a.T, in[j] & 0xFFFFFFu) | (SPB == 4 ? in[j] & 0xFF000000u : 0xFF000000u);
        if (c == 4 && ((uintptr_t)q & 3) == 0) {
            unsigned* d = (unsigned*)q;
            if (DPB == 4) {
#pragma unroll
                for (int j = 0; j < 4; ++j) d[j] = o[j];
            } else {
                d[0] = (o[0] & 0xFFFFFFu) | (o[1] << 24);
                d[1] = ((o[1] >> 8) & 0xFFFFu) | (o[2] << 16);
                d[2] = ((o[2] >> 16) & 0xFFu) | (o[3] << 8);
            }
        } else {
            for (int j = 0; j < c; ++j)
                for (int k = 0; k < DPB; ++k) q[j * DPB + k] = (unsigned char)(o[j] >> (8 * k));
        }
    }
}

int check_window(const char* who, const void* slide, long long pitch, int pixel_bytes, int H, int W, int x0, int y0, int w, int h) {
    if (!slide_args_ok(slide, pitch, pixel_bytes, H, W, who)) return HDY_EINVAL;
    HDY_ARG(H <= HDY_STAIN_MAX_SIDE && W <= HDY_STAIN_MAX_SIDE, "%s: slide of %d x %d pixels, a side above %d", who, H, W, HDY_STAIN_MAX_SIDE);
    HDY_ARG(x0 >= 0 && y0 >= 0 && w >= 1 && h >= 1 && (long long)x0 + w <= W && (long long)y0 + h <= H,
            "%s: the window (%d, %d) + %d x %d leaves the slide of %d x %d pixels", who, x0, y0, w, h, W, H);
    return HDY_OK;
}

// the walk of `threads` lanes per workgroup over the window's visited pixels, in at most max_blocks workgroups
int make_walk(Win& a, int& blocks, const unsigned char* slide, long long pitch, int x0, int y0, int w, int h, int step, int background, int threads,
              int max_blocks) {
    a.slide = slide; a.pitch = pitch; a.x0 = x0; a.y0 = y0; a.step = step; a.background = (unsigned)background;
    a.nx = (int)(((long long)w + step - 1) / step);
    a.ny = (int)(((long long)h + step - 1) / step);
    a.G = (a.nx + 3) / 4;
    a.items = (long long)a.G * a.ny;
    long long nb = (a.items + (long long)threads * ITEMS_PER_LANE - 1) / ((long long)threads * ITEMS_PER_LANE);
    nb = nb < 1 ? 1 : nb > max_blocks ? max_blocks : nb;
    a.chunk = (a.items + nb - 1) / nb;
    blocks = (int)((a.items + a.chunk - 1) / a.chunk);
    a.dr = threads / a.G;
    a.dg = threads % a.G;
    return HDY_OK;
}

// the checks the three counting passes share, then their walk
int count_args(const char* who, Win& a, int& blocks, const unsigned char* slide, long long pitch, int pixel_bytes, int H, int W, int x0, int y0, int w,
               int h, int step, int background, const void* ws, long long ws_bytes, long long cells, int max_blocks = MAX_BLOCKS) {
    HDY_CHECKED(check_window(who, slide, pitch, pixel_bytes, H, W, x0, y0, w, h));
    HDY_ARG(step >= 1, "%s: step=%d must be at least 1", who, step);
    HDY_ARG(background >= 0 && background <= 256, "%s: background %d (0 .. 256)", who, background);
    HDY_CHECKED(make_walk(a, blocks, slide, pitch, x0, y0, w, h, step, background, THREADS, max_blocks));
    HDY_ARG((long long)a.nx * a.ny <= (1ll << 40), "%s: %lld pixels to visit, at most 2^40 (raise step)", who, (long long)a.nx * a.ny);
    HDY_ARG(ws && ((uintptr_t)ws & 7) == 0, "%s: null or misaligned workspace pointer (ws 8 bytes)", who);
    HDY_ARG(ws_bytes >= (long long)MAX_BLOCKS * cells * 8, "%s: ws_bytes=%lld, the call needs HDY_STAIN_MAX_BLOCKS * %lld * 8 = %lld", who, ws_bytes,
            cells, (long long)MAX_BLOCKS * cells * 8);
    return HDY_OK;
}

void launch_reduce(const long long* slab, int rows, int cells, long long* out0, int n0, long long* out1, hipStream_t st) {
    hipLaunchKernelGGL(reduce_kernel, dim3((cells + 63) / 64), dim3(1024), 0, st, slab, rows, cells, out0, n0, out1);
}

template <bool ANGLES>
int launch_hist(const char* who, const Win& a, int blocks, int pixel_bytes, const int* lut, int bins, long long* hist, long long* skipped, void* ws,
                hipStream_t st) {
    const int cells = ANGLES ? bins + 1 : 2 * bins, stride = cells | 1;
    int copies = (HIST_LDS_BYTES - 1536 * 4) / (stride * 4);
    copies = copies > MAX_COPIES ? MAX_COPIES : copies;
    const size_t lds = (size_t)(1536 + copies * stride) * 4;
    if (pixel_bytes == 3)
        hipLaunchKernelGGL((hist_kernel<3, ANGLES>), dim3(blocks), dim3(THREADS), lds, st, a, lut, bins, cells, copies, (long long*)ws);
    else
        hipLaunchKernelGGL((hist_kernel<4, ANGLES>), dim3(blocks), dim3(THREADS), lds, st, a, lut, bins, cells, copies, (long long*)ws);
    HDY_LAUNCH_CHECK(who);
    launch_reduce((const long long*)ws, blocks, cells, hist, ANGLES ? bins : cells, skipped, st);
    HDY_LAUNCH_CHECK(who);
    return HDY_OK;
}

static_assert((HIST_LDS_BYTES - 1536 * 4) / (((2 * HDY_STAIN_MAX_BINS) | 1) * 4) >= 1, "the widest histogram fits beside the table");

}  // namespace

extern "C" {

int hdy_stain_revision(void) { return HDY_STAIN_REVISION; }

int hdy_stain_moments_u8(const unsigned char* slide, long long pitch_bytes, int pixel_bytes, int H, int W, int x0, int y0, int w, int h, int step,
                         int background, const int* od, long long od_elems, long long* sums, long long sums_elems, void* ws, long long ws_bytes,
                         void* stream) {
    const char* who = "stain_moments";
    Win a;
    int blocks;
    HDY_CHECKED(count_args(who, a, blocks, slide, pitch_bytes, pixel_bytes, H, W, x0, y0, w, h, step, background, ws, ws_bytes, 10));
    HDY_ARG(od && ((uintptr_t)od & 3) == 0, "%s: null or misaligned od pointer (4 bytes)", who);
    HDY_ARG(od_elems == 256, "%s: od_elems=%lld, the call reads 256", who, od_elems);
    HDY_ARG(sums && ((uintptr_t)sums & 7) == 0, "%s: null or misaligned sums pointer (8 bytes)", who);
    HDY_ARG(sums_elems == 10, "%s: sums_elems=%lld, the call writes 10", who, sums_elems);
    hipStream_t st = (hipStream_t)stream;
    if (pixel_bytes == 3) hipLaunchKernelGGL(moments_kernel<3>, dim3(blocks), dim3(THREADS), 0, st, a, od, (long long*)ws);
    else hipLaunchKernelGGL(moments_kernel<4>, dim3(blocks), dim3(THREADS), 0, st, a, od, (long long*)ws);
    HDY_LAUNCH_CHECK(who);
    launch_reduce((const long long*)ws, blocks, 10, sums, 10, sums, st);
    HDY_LAUNCH_CHECK(who);
    hdy_note_dispatch("stain_moments");
    return HDY_OK;
}

int hdy_stain_angles_u8(const unsigned char* slide, long long pitch_bytes, int pixel_bytes, int H, int W, int x0, int y0, int w, int h, int step,
                        int background, const int* lut, long long lut_elems, int A, long long* hist, long long hist_elems, long long* skipped,
                        long long skipped_elems, void* ws, long long ws_bytes, void* stream) {
    const char* who = "stain_angles";
    HDY_ARG(A >= 1 && A <= HDY_STAIN_MAX_BINS, "%s: A=%d outside [1, %d]", who, A, HDY_STAIN_MAX_BINS);
    Win a;
    int blocks;
    HDY_CHECKED(count_args(who, a, blocks, slide, pitch_bytes, pixel_bytes, H, W, x0, y0, w, h, step, background, ws, ws_bytes, A + 1, HIST_MAX_BLOCKS));
    HDY_ARG(lut && ((uintptr_t)lut & 3) == 0, "%s: null or misaligned lut pointer (4 bytes)", who);
    HDY_ARG(lut_elems == 1536, "%s: lut_elems=%lld, the call reads 2 * 3 * 256 = 1536", who, lut_elems);
    HDY_ARG(hist && skipped && (((uintptr_t)hist | (uintptr_t)skipped) & 7) == 0, "%s: null or misaligned hist or skipped pointer (8 bytes)", who);
    HDY_ARG(hist_elems == A, "%s: hist_elems=%lld, the call writes A = %d", who, hist_elems, A);
    HDY_ARG(skipped_elems == 1, "%s: skipped_elems=%lld, the call writes 1", who, skipped_elems);
    HDY_CHECKED(launch_hist<true>(who, a, blocks, pixel_bytes, lut, A, hist, skipped, ws, (hipStream_t)stream));
    hdy_note_dispatch("stain_angles");
    return HDY_OK;
}

int hdy_stain_levels_u8(const unsigned char* slide, long long pitch_bytes, int pixel_bytes, int H, int W, int x0, int y0, int w, int h, int step,
                        int background, const int* lut, long long lut_elems, int B, long long* hist, long long hist_elems, void* ws,
                        long long ws_bytes, void* stream) {
    const char* who = "stain_levels";
    HDY_ARG(B >= 1 && B <= HDY_STAIN_MAX_BINS, "%s: B=%d outside [1, %d]", who, B, HDY_STAIN_MAX_BINS);
    Win a;
    int blocks;
    HDY_CHECKED(count_args(who, a, blocks, slide, pitch_bytes, pixel_bytes, H, W, x0, y0, w, h, step, background, ws, ws_bytes, 2ll * B, HIST_MAX_BLOCKS));
    HDY_ARG(lut && ((uintptr_t)lut & 3) == 0, "%s: null or misaligned lut pointer (4 bytes)", who);
    HDY_ARG(lut_elems == 1536, "%s: lut_elems=%lld, the call reads 2 * 3 * 256 = 1536", who, lut_elems);
    HDY_ARG(hist && ((uintptr_t)hist & 7) == 0, "%s: null or misaligned hist pointer (8 bytes)", who);
    HDY_ARG(hist_elems == 2ll * B, "%s: hist_elems=%lld, the call writes 2 * B = 2 * %d", who, hist_elems, B);
    HDY_CHECKED(launch_hist<false>(who, a, blocks, pixel_bytes, lut, B, hist, hist, ws, (hipStream_t)stream));
    hdy_note_dispatch("stain_levels");
    return HDY_OK;
}

int hdy_stain_apply_u8(const unsigned char* slide, long long pitch_bytes, int pixel_bytes, int H, int W, int x0, int y0, int w, int h,
                       unsigned char* dst, long long dst_pitch, int dst_pixel_bytes, const int* lut, long long lut_elems,
                       const unsigned char* tone, long long tone_elems, int T, void* stream) {
    const char* who = "stain_apply";
    HDY_CHECKED(check_window(who, slide, pitch_bytes, pixel_bytes, H, W, x0, y0, w, h));
    HDY_ARG(dst, "%s: null dst pointer", who);
    HDY_ARG(dst_pixel_bytes == 3 || dst_pixel_bytes == 4, "%s: dst_pixel_bytes is %d, 3 (RGB) or 4 (RGBA) expected", who, dst_pixel_bytes);
    HDY_ARG(dst_pitch >= (long long)W * dst_pixel_bytes, "%s: dst_pitch of %lld bytes is below W * dst_pixel_bytes = %lld", who, dst_pitch,
            (long long)W * dst_pixel_bytes);
    HDY_ARG(pitch_bytes <= (1ll << 32) && dst_pitch <= (1ll << 32), "%s: a row pitch above 2^32 bytes (%lld, %lld)", who, pitch_bytes, dst_pitch);
    {
        const uintptr_t s0 = (uintptr_t)slide, s1 = s0 + (uintptr_t)(H - 1) * pitch_bytes + (uintptr_t)W * pixel_bytes;
        const uintptr_t d0 = (uintptr_t)dst, d1 = d0 + (uintptr_t)(H - 1) * dst_pitch + (uintptr_t)W * dst_pixel_bytes;
        const bool same = d0 == s0 && dst_pitch == pitch_bytes && dst_pixel_bytes == pixel_bytes;
        HDY_ARG(same || d1 <= s0 || s1 <= d0, "%s: dst overlaps the slide without being the slide itself (same pointer, pitch and pixel_bytes)", who);
    }
    HDY_ARG(T >= 1 && T <= HDY_STAIN_MAX_TONE, "%s: T=%d outside [1, %d]", who, T, HDY_STAIN_MAX_TONE);
    HDY_ARG(lut && ((uintptr_t)lut & 3) == 0, "%s: null or misaligned lut pointer (4 bytes)", who);
    HDY_ARG(lut_elems == 2304, "%s: lut_elems=%lld, the call reads 3 * 3 * 256 = 2304", who, lut_elems);
    HDY_ARG(tone, "%s: null tone pointer", who);
    HDY_ARG(tone_elems == T, "%s: tone_elems=%lld, the call reads T = %d", who, tone_elems, T);
    ApplyArgs a;
    int blocks;
    HDY_CHECKED(make_walk(a.win, blocks, slide, pitch_bytes, x0, y0, w, h, 1, 0, APPLY_THREADS, APPLY_MAX_BLOCKS));
    a.dst = dst; a.dst_pitch = dst_pitch; a.lut = lut; a.tone = tone; a.T = T;
    hipStream_t st = (hipStream_t)stream;
#define HDY_STAIN_APPLY(S, D) hipLaunchKernelGGL((apply_kernel<S, D>), dim3(blocks), dim3(APPLY_THREADS), 0, st, a)
    if (pixel_bytes == 3 && dst_pixel_bytes == 3) HDY_STAIN_APPLY(3, 3);
    else if (pixel_bytes == 3) HDY_STAIN_APPLY(3, 4);
    else if (dst_pixel_bytes == 3) HDY_STAIN_APPLY(4, 3);
    else HDY_STAIN_APPLY(4, 4);
#undef HDY_STAIN_APPLY
    HDY_LAUNCH_CHECK(who);
    hdy_note_dispatch("stain_apply");
    return HDY_OK;
}

}  // extern "C"
