// Per-label measurements of a slide label map (hdy_label_measure): one streaming pass over the int32 map and, optionally, the 8-bit slide
// under it leaves per label 14 exact integer sums (count, first and second moments, boundary edges, border edges, stain sums) and the extent.
// Integer work bound by loads, LDS and atomics; no MFMA, no LDS-DMA.
//
// The arithmetic is stated in include/hdyolo_measure.h and restated in tests/measure_ref.py.
//
// measure_kernel: every wave works alone, on strips of ROWS x TW = 8 x 64 map entries (a workgroup's four waves take the four strips of one
// 32 x 64 tile, so their halo rows meet in the cache; a grid-stride walk over the tiles, 64-bit tile index; no workgroup barrier).  The strip is
// staged in the wave's own LDS with a one-entry halo, a map row per load (entries outside the window as -1, which differs from every label),
// and while those loads are in flight every lane loads the three colour bytes of its 8 pixels (lanes on consecutive pixels: one contiguous
// row segment of 192 / 256 bytes per row).  The wave then walks its 8 rows, lane = column:
//   - the runs of equal labels of the 64 entries come from one ballot, as in paste.hip's areas_kernel;
//   - everything geometric about a run is a closed form of (first column, row, length) in STRIP coordinates: n, sum x, sum y, sum x^2,
//     sum y^2, sum x * y; the boundary edges of the run are four popcounts of neighbour-differs ballots under the run's lane mask, the edges
//     that leave the window follow from the run's ends;
//   - the six stain sums are the difference of a wave-wide inclusive scan (five words: R | G << 16, B, R^2, G^2, B^2; six DPP adds each)
//     between the run's last and first lane;
//   - the first lane of a run of a label adds the values (32-bit: a strip holds 512 entries) to the label's row of the wave's 16-slot LDS
//     table (open addressing, key claimed by an LDS compare-and-swap) and folds the run into the row's extent.
// Then the table is flushed, slot by used slot, lane = column or extent entry: the strip-relative moments are moved to the label's origin,
//     sum dx = sum x + n a,  sum dx^2 = sum x^2 + 2 a sum x + n a^2,  sum dx dy = sum x y + a sum y + b sum x + n a b   (a = strip x0 - ox, b alike)
// which is exact modulo 2^64 whatever the origin, and added with one 64-bit global atomicAdd per non-zero (label, column), 14 neighbouring
// lanes on one 112-byte row, plus an atomicMin / atomicMax per extent entry.  A run that finds the table full does the same move and goes
// straight to global atomics.  A row without a label skips everything behind its first ballot; a strip without one issues no atomic.
// Measured (profiles/measure_ab.txt): the pass is bound by instruction issue, not by HBM; the workgroup-wide form with
// barriers and a shuffle scan that came first took 1.55 x as long.
//
// Contract: no allocation, everything on the passed stream, no host synchronisation; all argument checks before any launch.
#include "label_common.h"
#include "hdyolo_measure.h"

namespace {

typedef unsigned long long u64;

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int TW = 64, TH = 32;                  // a workgroup's tile: one strip of ROWS map rows per wave, a strip row = one wave row
constexpr int ROWS = TH / WAVES;                 // map rows per strip
constexpr int LW = TW + 2, SH = ROWS + 2;        // a strip with its halo
constexpr int SLOTS = 16;                        // rows of a wave's LDS table (a power of two)
constexpr int COLS = HDY_MEASURE_COLS;
constexpr int OUTS = COLS + 4;                   // columns + extent entries: the flush's items per slot
constexpr int MAX_BLOCKS = 1 << 16;
static_assert(COLS == 14 && (SLOTS & (SLOTS - 1)) == 0 && ROWS * WAVES == TH && OUTS <= 64, "layout");

struct Args {
    const int* map;
    int h, w;
    Image im;                                    // im.img null: no stain sums
    const int* origin;
    u64* sums;
    int* extent;
    int R;
    long long tiles;
    int tiles_x;
};

// column c of a label's row about its origin from the row about the strip's corner: a = strip x0 - ox, b = strip y0 - oy, modulo 2^64
template <typename V> __device__ __forceinline__ u64 moved(int c, const V& v, u64 a, u64 b) {
    // v[c] + a * alpha + b * beta with the column's alpha and beta selected, not branched to: two 64-bit products for any column
    const u64 n = v[0], sx = v[1], sy = v[2];
    const u64 na = n * a, nb = n * b;
    const u64 alpha = c == 1 ? n : c == 3 ? 2 * sx + na : c == 5 ? sy + nb : 0;
    const u64 beta = c == 2 ? n : c == 4 ? 2 * sy + nb : c == 5 ? sx : 0;
    return v[c] + a * alpha + b * beta;
}

__device__ __forceinline__ void origin_shift(const Args& a, int r, int i0, int j0, u64& sa, u64& sb) {
    long long ox = 0, oy = 0;
    if (a.origin) {
        ox = a.origin[2 * (size_t)r];
        oy = a.origin[2 * (size_t)r + 1];
    }
    sa = (u64)((long long)j0 - ox);
    sb = (u64)((long long)i0 - oy);
}

__device__ __forceinline__ int slot_of(int* keys, int r) {
    unsigned s = ((unsigned)r * 0x9E3779B1u) >> 28;          // Fibonacci hashing into 16 slots
    static_assert(SLOTS == 16, "hash width");
    for (int probe = 0; probe < SLOTS; ++probe, s = (s + 1) & (SLOTS - 1)) {
        int cur = keys[s];
        if (cur == -1) {
            cur = atomicCAS(&keys[s], -1, r);
            if (cur == -1) cur = r;
        }
        if (cur == r) return (int)s;
    }
    return -1;
}

// inclusive prefix sum over the 64 lanes in six DPP adds: shifts by 1, 2, 4, 8 inside each row of 16 lanes (lanes without a source add the
// `old` operand, 0), then lane 15 of rows 0 and 2 onto rows 1 and 3 (row_bcast:15, row mask 0xA), then lane 31 onto rows 2 and 3 (row_bcast:31, 0xC)
__device__ __forceinline__ unsigned wave_scan(unsigned u) {
    int v = (int)u;
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, false);      // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, false);      // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, false);      // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, false);      // row_shr:8
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, false);      // row_bcast:15
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, false);      // row_bcast:31
    return (unsigned)v;
}

__global__ __launch_bounds__(THREADS) void init_kernel(u64* __restrict__ sums, int* __restrict__ extent, int R, int h, int w) {
    const long long stride = (long long)gridDim.x * THREADS;
    for (long long i = (long long)blockIdx.x * THREADS + threadIdx.x; i < (long long)R * COLS; i += stride) sums[i] = 0;
    for (long long i = (long long)blockIdx.x * THREADS + threadIdx.x; i < (long long)R * 4; i += stride)
        extent[i] = (i & 3) == 0 ? w : (i & 3) == 1 ? h : -1;
}

__global__ __launch_bounds__(THREADS) void measure_kernel(const Args a) {
    __shared__ int tile_s[WAVES][SH * LW];
    __shared__ int keys_s[WAVES][SLOTS];
    __shared__ u64 vals_s[WAVES][SLOTS * COLS / 2];          // columns 2p | 2p + 1 << 32: one 64-bit LDS add per pair, no carry (32-bit sums)
    __shared__ int ext_s[WAVES][SLOTS * 4];                  // per slot: min j, max j, bit k = the label owns entries of strip row k, unused
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    // everything below is private to the wave: no workgroup barrier anywhere.  A wave's LDS operations complete in program order, so the fences
    // only keep the compiler from moving them across the points where lanes read what other lanes of the wave wrote.
    int* tile = tile_s[wv];
    int* keys = keys_s[wv];
    u64* vals = vals_s[wv];
    const unsigned* vals32 = (const unsigned*)vals;          // column c of slot s at [s * COLS + c]
    int* ext = ext_s[wv];

    for (long long tl = blockIdx.x; tl < a.tiles; tl += gridDim.x) {
        const long long ty = tl / a.tiles_x;
        const int i0 = (int)ty * TH + wv * ROWS, j0 = (int)(tl - ty * a.tiles_x) * TW;       // < 2^29 + tile
        if (i0 >= a.h) continue;                                                 // wave-uniform: the tile's last strips may lie below the window

        // ---- an empty table, the strip with its halo, the pixels
#pragma unroll
        for (int it = 0; it < (SLOTS * COLS / 2 + 63) / 64; ++it)
            if (lane + it * 64 < SLOTS * COLS / 2) vals[lane + it * 64] = 0;
        if (lane < SLOTS) {
            keys[lane] = -1;
            ext[4 * lane] = 0x7fffffff; ext[4 * lane + 1] = -1; ext[4 * lane + 2] = 0;
        }
        const bool col_in = j0 + lane < a.w;
#pragma unroll
        for (int ly = 0; ly < SH; ++ly) {                                        // a row of the strip per load, all SH loads in flight at once
            const int gi = i0 + ly - 1;
            tile[ly * LW + lane + 1] = (gi >= 0 && gi < a.h && col_in) ? a.map[(long long)gi * a.w + j0 + lane] : -1;
        }
        if (lane < 2 * SH) {                                                     // the halo's two columns
            const int ly = lane >> 1, lx = (lane & 1) * (LW - 1);
            const int gi = i0 + ly - 1, gj = j0 + lx - 1;
            tile[ly * LW + lx] = (gi >= 0 && gi < a.h && gj >= 0 && gj < a.w) ? a.map[(long long)gi * a.w + gj] : -1;
        }
        unsigned px[ROWS];
        if (a.im.img) {
#pragma unroll
            for (int k = 0; k < ROWS; ++k) {
                const int gi = i0 + k, gj = j0 + lane;
                px[k] = 0;
                if (gi < a.h && gj < a.w) {
                    const unsigned char* p = a.im.pixel(gi, gj);
                    px[k] = (unsigned)p[0] | (unsigned)p[1] << 8 | (unsigned)p[2] << 16;
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");

        // ---- the strip's rows
        bool any = false;                                                        // wave-uniform: the strip holds a label
#pragma unroll
        for (int k = 0; k < ROWS; ++k) {
            const int gi = i0 + k, gj = j0 + lane;
            if (gi >= a.h) break;                                                // wave-uniform
            const int* row = tile + (k + 1) * LW + lane + 1;
            const int c = row[0];
            const bool valid = (unsigned)c < (unsigned)a.R;                      // entries beyond the window hold -1
            if (__ballot(valid) == 0) continue;                                  // wave-uniform: a row of background
            any = true;
            const int prev = __shfl_up(c, 1);
            const bool head = lane == 0 || c != prev;
            const u64 heads = __ballot(head);
            const u64 rest = lane == 63 ? 0ull : heads >> (lane + 1);
            const int L = rest ? __ffsll((unsigned long long)rest) : 64 - lane;  // from this lane to the end of its run
            const u64 m = (L == 64 ? ~0ull : (1ull << L) - 1) << lane;
            const int edges = __popcll(__ballot(row[-LW] != c) & m) + __popcll(__ballot(row[LW] != c) & m) +
                              __popcll(__ballot(row[-1] != c) & m) + __popcll(__ballot(row[1] != c) & m);
            unsigned st[5] = {0, 0, 0, 0, 0};                                    // the run's R | G << 16, B, R^2, G^2, B^2 sums (first lane)
            if (a.im.img) {                                                      // kernel-uniform
                const unsigned p = valid ? px[k] : 0u;
                const unsigned cr = p & 255u, cg = (p >> 8) & 255u, cb = p >> 16;
                // wave-wide sums: colour <= 64 * 255 < 2^16, square <= 64 * 255^2 < 2^32: neither the packed fields nor the words overflow
                const unsigned own[5] = {cr | cg << 16, cb, cr * cr, cg * cg, cb * cb};
                const int tail = lane + L - 1;                                   // <= 63: the last lane of this lane's run
#pragma unroll
                for (int q = 0; q < 5; ++q) {
                    const unsigned pre = wave_scan(own[q]);
                    st[q] = (unsigned)__shfl((int)pre, tail) - pre + own[q];
                }
            }
            if (head && valid) {
                const unsigned n = (unsigned)L, x = (unsigned)lane, y = (unsigned)k;
                const unsigned tri = n * (n - 1) / 2, sq = (n - 1) * n * (2 * n - 1) / 6;       // sum k, sum k^2 over k < n
                unsigned v[COLS];
                v[0] = n;
                v[1] = n * x + tri;
                v[2] = n * y;
                v[3] = n * x * x + 2 * x * tri + sq;
                v[4] = n * y * y;
                v[5] = y * v[1];
                v[6] = (unsigned)edges;
                v[7] = n * ((gi == 0) + (gi == a.h - 1)) + (gj == 0) + (gj + L - 1 == a.w - 1);
                v[8] = st[0] & 0xFFFFu;
                v[9] = st[0] >> 16;
                v[10] = st[1];
                v[11] = st[2];
                v[12] = st[3];
                v[13] = st[4];
                const int s = slot_of(keys, c);
                if (s >= 0) {
#pragma unroll
                    for (int q = 0; q < COLS / 2; ++q)
                        if (q < 4 || a.im.img) atomicAdd(&vals[s * (COLS / 2) + q], (u64)v[2 * q] | (u64)v[2 * q + 1] << 32);
                    atomicMin(&ext[4 * s], gj);
                    atomicMax(&ext[4 * s + 1], gj + L - 1);
                    atomicOr(&ext[4 * s + 2], 1 << k);
                } else {                                                         // table full: this run goes to global memory itself
                    u64 sa, sb;
                    origin_shift(a, c, i0, j0, sa, sb);
#pragma unroll
                    for (int q = 0; q < COLS; ++q) {
                        const u64 val = moved(q, v, sa, sb);
                        if (val) atomicAdd(&a.sums[(size_t)c * COLS + q], val);
                    }
                    atomicMin(&a.extent[4 * (size_t)c], gj);
                    atomicMin(&a.extent[4 * (size_t)c + 1], gi);
                    atomicMax(&a.extent[4 * (size_t)c + 2], gj + L - 1);
                    atomicMax(&a.extent[4 * (size_t)c + 3], gi);
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        if (!any) continue;                                                      // nothing but background: no atomic, and the table is still empty

        // ---- flush: per used slot, lane = column or extent entry
        u64 used = __ballot(lane < SLOTS && keys[lane < SLOTS ? lane : 0] >= 0);
        while (used) {
            const int s = __ffsll((unsigned long long)used) - 1;
            used &= used - 1;
            const int r = keys[s];
            if (lane < COLS) {
                u64 sa, sb;
                origin_shift(a, r, i0, j0, sa, sb);
                const u64 val = moved(lane, vals32 + s * COLS, sa, sb);
                if (val) atomicAdd(&a.sums[(size_t)r * COLS + lane], val);
            } else if (lane < OUTS) {
                const int rows = ext[4 * s + 2];                                 // not 0: the slot is used
                if (lane == COLS) atomicMin(&a.extent[4 * (size_t)r], ext[4 * s]);
                else if (lane == COLS + 1) atomicMin(&a.extent[4 * (size_t)r + 1], i0 + __ffs(rows) - 1);
                else if (lane == COLS + 2) atomicMax(&a.extent[4 * (size_t)r + 2], ext[4 * s + 1]);
                else atomicMax(&a.extent[4 * (size_t)r + 3], i0 + 31 - __clz(rows));
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");                   // the table is read before the next strip empties it
        __builtin_amdgcn_wave_barrier();
    }
}

}  // namespace

extern "C" {

int hdy_measure_revision(void) { return HDY_MEASURE_REVISION; }

int hdy_label_measure(const int* map, long long map_elems, int h, int w, const unsigned char* image, long long image_bytes, long long row_stride,
                      int pixel_stride, int x0, int y0, const int* origin, long long* sums, long long sums_elems, int* extent,
                      long long extent_elems, int R, void* stream) {
    const char* who = "label_measure";
    HDY_ARG(sums_elems >= 0, "%s: negative count (sums_elems=%lld)", who, sums_elems);
    HDY_CHECKED(check_map(who, map_elems, h, w, HDY_MEASURE_MAX_SIDE));
    HDY_CHECKED(check_extent(who, extent_elems, R, "writes"));
    HDY_ARG(sums_elems == (long long)HDY_MEASURE_COLS * R, "%s: sums_elems=%lld, the call writes %d * R = %d * %d", who, sums_elems,
            HDY_MEASURE_COLS, HDY_MEASURE_COLS, R);
    HDY_ARG(R == 0 || (map && sums && extent), "%s: null map, sums or extent pointer", who);
    HDY_ARG(((uintptr_t)sums & 7) == 0 && (((uintptr_t)map | (uintptr_t)origin | (uintptr_t)extent) & 3) == 0,
            "%s: misaligned pointer (sums 8 bytes; map, origin, extent 4 bytes)", who);
    if (image) HDY_CHECKED(check_image(who, h, w, image_bytes, row_stride, pixel_stride, x0, y0));
    if (R == 0) return HDY_OK;
    hipStream_t st = (hipStream_t)stream;
    Args a = {};
    a.map = map; a.h = h; a.w = w; a.im = {image, row_stride, pixel_stride, x0, y0};
    a.origin = origin; a.sums = (u64*)sums; a.extent = extent; a.R = R;
    a.tiles_x = (w + TW - 1) / TW;
    a.tiles = (long long)a.tiles_x * ((h + TH - 1) / TH);
    const long long init_blocks = ((long long)R * COLS + THREADS - 1) / THREADS;
    hipLaunchKernelGGL(init_kernel, dim3((unsigned)(init_blocks < 4096 ? init_blocks : 4096)), dim3(THREADS), 0, st, a.sums, extent, R, h, w);
    hipLaunchKernelGGL(measure_kernel, dim3((unsigned)(a.tiles < MAX_BLOCKS ? a.tiles : MAX_BLOCKS)), dim3(THREADS), 0, st, a);
    HDY_LAUNCH_CHECK(who);
    hdy_note_dispatch("label_measure");
    return HDY_OK;
}

}  // extern "C"
