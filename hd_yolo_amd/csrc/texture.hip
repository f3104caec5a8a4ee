// Texture counts of every label of a slide label map (hdy_label_texture): from the int32 map, the 8-bit slide under it and the extents of
// hdy_label_measure the pass leaves per label the histogram of quantised levels and one symmetric grey-level co-occurrence matrix per offset.
// Integer work bound by loads and LDS atomics; no MFMA, no LDS-DMA.
//
// The arithmetic is stated in include/hdyolo_texture.h and restated in tests/texture_ref.py.
//
// texture_kernel<L, THREADS>: the workgroup copies the 3 KB level table to LDS once (the kernel's only workgroup barrier, before any wave
// leaves the common path); from there every wave works alone, on one label at a time (grid-stride over the call's rows).  The wave keeps the
// label's histogram and its MAXD matrices in its own LDS ((MAXD * L * L + L) words: 1 KB, 4 KB, 16 KB at L = 8, 16, 32), so THREADS is 256 up
// to L = 16 and 128 at L = 32 and every instance stays below 64 KB of static LDS.  It walks the clamped box in steps of 64 entries: boxes of
// 64 columns and more a row segment of 64 columns per step, narrower ones 64 / cw rows of cw columns (cw = the power of two at or above the
// box width), so that a nucleus of 20 x 20 entries keeps 40 of the 64 lanes busy and not 20.  A lane whose entry holds the label computes its
// level from three table reads, adds to the histogram and, per offset, looks at the neighbour's map entry, recomputes the neighbour's level
// from the image (the pixel loads hit the cache: the neighbour is at most 4 entries away) and adds to the two mirror cells with LDS atomics,
// or 2 to the diagonal cell.  The finished table goes out with plain coalesced stores; a flagged label stores zeros.
//
// Contract: no allocation, everything on the passed stream, no host synchronisation; all argument checks before any launch.
#include "label_common.h"
#include "hdyolo_texture.h"

namespace {

constexpr int MAXD = HDY_TEXTURE_MAX_OFFSETS;
constexpr int MAX_SIDE = HDY_TEXTURE_MAX_SIDE;
constexpr int SHIFT = HDY_TEXTURE_SHIFT;
constexpr int MAX_BLOCKS = 4096;                 // a grid-stride walk over the labels: enough workgroups to fill every CU several times
static_assert(MAXD == 4 && HDY_TEXTURE_MAX_LEVELS == 32, "the LDS budget below is written for 4 offsets and 32 levels");

struct Args {
    const int* map;
    int h, w;
    Image im;
    const int* extent;
    const int* lut;
    int D;
    int di[MAXD], dj[MAXD];
    int row0, rows;
    int* hist;
    int* glcm;
    int* flags;
};

template <int L> __device__ __forceinline__ int level_of(const Args& a, const int* lut, int i, int j) {
    const unsigned char* p = a.im.pixel(i, j);
    const unsigned t = (unsigned)lut[p[0]] + (unsigned)lut[256 + p[1]] + (unsigned)lut[512 + p[2]];       // modulo 2^32
    const int v = (int)t >> SHIFT;                                                                         // floor(t / 2^SHIFT)
    return v < 0 ? 0 : v > L - 1 ? L - 1 : v;
}

template <int L, int THREADS> __global__ __launch_bounds__(THREADS) void texture_kernel(const Args a) {
    constexpr int WAVES = THREADS / 64;
    constexpr int CELLS = MAXD * L * L + L;                  // the matrices, then the histogram
    __shared__ int lut_s[768];
    __shared__ int acc_s[WAVES][CELLS];
    static_assert(sizeof(int) * (768 + WAVES * CELLS) <= 64 * 1024, "static LDS");
    for (int k = threadIdx.x; k < 768; k += THREADS) lut_s[k] = a.lut[k];
    __syncthreads();
    // everything below is private to the wave: no workgroup barrier.  A wave's LDS operations complete in program order, so the fences only
    // keep the compiler from moving them across the points where lanes read what other lanes of the wave wrote.
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int* acc = acc_s[wv];
    int* hist = acc + MAXD * L * L;
    const int used = a.D * L * L;                            // cells of the matrices this call writes

    for (long long q = (long long)blockIdx.x * WAVES + wv; q < a.rows; q += (long long)gridDim.x * WAVES) {
        const int r = a.row0 + (int)q;
        const Box b = clamped_box(a.extent, r, a.h, a.w, MAX_SIDE);
        int* gq = a.glcm + (size_t)q * used;
        int* hq = a.hist + (size_t)q * L;
        if (lane == 0) a.flags[q] = b.flag;
        if (b.flag) {                                        // wave-uniform
            for (int k = lane; k < used; k += 64) gq[k] = 0;
            if (lane < L) hq[lane] = 0;
            continue;
        }
        for (int k = lane; k < CELLS; k += 64) acc[k] = 0;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");

        int sh = 6;                                          // cw = 1 << sh columns per step, 64 >> sh rows
        while (sh > 0 && (1 << (sh - 1)) >= b.bw) --sh;
        const int cw = 1 << sh, rp = 64 >> sh;
        const int li = lane >> sh, lj = lane & (cw - 1);
        const int bx1 = b.x0 + b.bw - 1, by1 = b.y0 + b.bh - 1;
        for (int ib = b.y0; ib <= by1; ib += rp) {
            const int i = ib + li;
            for (int jb = b.x0; jb <= bx1; jb += cw) {
                const int j = jb + lj;
                if (i > by1 || j > bx1 || a.map[(long long)i * a.w + j] != r) continue;      // inside the window: the box is clamped
                const int lv = level_of<L>(a, lut_s, i, j);
                atomicAdd(&hist[lv], 1);
#pragma unroll
                for (int d = 0; d < MAXD; ++d) {                                 // unrolled: the offsets stay in scalar registers
                    if (d >= a.D) break;
                    const int ni = i + a.di[d], nj = j + a.dj[d];
                    if (!owns(a.map, a.h, a.w, ni, nj, r)) continue;
                    const int nl = level_of<L>(a, lut_s, ni, nj);
                    int* m = acc + d * L * L;
                    if (nl == lv) {
                        atomicAdd(&m[lv * L + lv], 2);
                    } else {
                        atomicAdd(&m[lv * L + nl], 1);
                        atomicAdd(&m[nl * L + lv], 1);
                    }
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        for (int k = lane; k < used; k += 64) gq[k] = acc[k];
        if (lane < L) hq[lane] = hist[lane];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");                   // the table is read before the next label empties it
        __builtin_amdgcn_wave_barrier();
    }
}

template <int L, int THREADS> void launch(const Args& a, hipStream_t st) {
    hipLaunchKernelGGL((texture_kernel<L, THREADS>), dim3(label_blocks(a.rows, THREADS / 64, MAX_BLOCKS)), dim3(THREADS), 0, st, a);
}

}  // namespace

extern "C" {

int hdy_texture_revision(void) { return HDY_TEXTURE_REVISION; }

int hdy_label_texture(const int* map, long long map_elems, int h, int w, const unsigned char* image, long long image_bytes, long long row_stride,
                      int pixel_stride, int x0, int y0, const int* extent, long long extent_elems, int R, const int* lut, long long lut_elems,
                      int levels, const int* offsets, long long offsets_elems, int D, int row0, int rows, int* hist, long long hist_elems,
                      int* glcm, long long glcm_elems, int* flags, long long flags_elems, void* stream) {
    const char* who = "label_texture";
    HDY_ARG(lut_elems >= 0 && offsets_elems >= 0 && hist_elems >= 0 && glcm_elems >= 0 && flags_elems >= 0,
            "%s: negative count (lut_elems=%lld, offsets_elems=%lld, hist_elems=%lld, glcm_elems=%lld, flags_elems=%lld)", who, lut_elems,
            offsets_elems, hist_elems, glcm_elems, flags_elems);
    HDY_CHECKED(check_map(who, map_elems, h, w, HDY_TEXTURE_MAX_WINDOW));
    HDY_CHECKED(check_extent(who, extent_elems, R, "reads"));
    HDY_ARG(lut_elems == 768, "%s: lut_elems=%lld, the call reads 3 * 256 = 768", who, lut_elems);
    HDY_ARG(levels == 8 || levels == 16 || levels == 32, "%s: levels=%d (8, 16 or 32)", who, levels);
    HDY_ARG(D >= 1 && D <= HDY_TEXTURE_MAX_OFFSETS, "%s: D=%d outside [1, %d]", who, D, HDY_TEXTURE_MAX_OFFSETS);
    HDY_ARG(offsets_elems == 2ll * D, "%s: offsets_elems=%lld, the call reads 2 * D = 2 * %d", who, offsets_elems, D);
    HDY_ARG(offsets, "%s: null offsets pointer (a host array of D pairs (di, dj))", who);
    HDY_ARG(((uintptr_t)offsets & 3) == 0, "%s: misaligned pointer (offsets 4 bytes)", who);
    for (int d = 0; d < D; ++d) {
        const int di = offsets[2 * d], dj = offsets[2 * d + 1];
        HDY_ARG(di >= -HDY_TEXTURE_MAX_REACH && di <= HDY_TEXTURE_MAX_REACH && dj >= -HDY_TEXTURE_MAX_REACH && dj <= HDY_TEXTURE_MAX_REACH,
                "%s: offsets[%d]=(%d, %d) reaches beyond %d", who, d, di, dj, HDY_TEXTURE_MAX_REACH);
        HDY_ARG(di != 0 || dj != 0, "%s: offsets[%d]=(0, 0) pairs an entry with itself", who, d);
    }
    HDY_ARG(row0 >= 0 && rows >= 0, "%s: negative row0=%d or rows=%d", who, row0, rows);
    HDY_ARG((long long)row0 + rows <= R, "%s: row0 + rows = %d + %d passes R=%d", who, row0, rows, R);
    HDY_ARG(hist_elems == (long long)rows * levels, "%s: hist_elems=%lld, the call writes rows * levels = %d * %d", who, hist_elems, rows, levels);
    HDY_ARG(glcm_elems == (long long)rows * D * levels * levels, "%s: glcm_elems=%lld, the call writes rows * D * levels^2 = %d * %d * %d^2", who,
            glcm_elems, rows, D, levels);
    HDY_ARG(flags_elems == rows, "%s: flags_elems=%lld, the call writes rows = %d", who, flags_elems, rows);
    HDY_ARG(rows == 0 || (map && extent && lut), "%s: null map, extent or lut pointer", who);
    HDY_ARG(rows == 0 || image, "%s: null image pointer (the pass reads the pixels under the map)", who);
    HDY_ARG(rows == 0 || (hist && glcm && flags), "%s: null hist, glcm or flags pointer", who);
    HDY_ARG((((uintptr_t)map | (uintptr_t)extent | (uintptr_t)lut | (uintptr_t)hist | (uintptr_t)glcm | (uintptr_t)flags) & 3) == 0,
            "%s: misaligned pointer (map, extent, lut, hist, glcm, flags 4 bytes)", who);
    HDY_CHECKED(check_image(who, h, w, image_bytes, row_stride, pixel_stride, x0, y0));
    if (R == 0 || rows == 0) return HDY_OK;
    hipStream_t st = (hipStream_t)stream;
    Args a = {};
    a.map = map; a.h = h; a.w = w; a.im = {image, row_stride, pixel_stride, x0, y0};
    a.extent = extent; a.lut = lut; a.D = D; a.row0 = row0; a.rows = rows; a.hist = hist; a.glcm = glcm; a.flags = flags;
    for (int d = 0; d < MAXD; ++d) {
        a.di[d] = offsets[2 * (d < D ? d : D - 1)];
        a.dj[d] = offsets[2 * (d < D ? d : D - 1) + 1];
    }
    if (levels == 8) launch<8, 256>(a, st);
    else if (levels == 16) launch<16, 256>(a, st);
    else launch<32, 128>(a, st);
    HDY_LAUNCH_CHECK(who);
    hdy_note_dispatch("label_texture");
    return HDY_OK;
}

}  // extern "C"
