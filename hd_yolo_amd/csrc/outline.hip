// Outline polygons and convex-hull descriptors of the labels of a slide label map (hdy_label_outline_count, hdy_label_outline_write,
// hdy_label_hull): from the int32 map and the extents of hdy_label_measure to a vertex list per label and to hull area, perimeter and the
// two Feret diameters.  Integer work bound by dependent loads; no MFMA, no LDS-DMA, no atomics except the one status word.
//
// The geometry and the arithmetic are stated in include/hdyolo_outline.h and restated in tests/outline_ref.py.
//
// walk_kernel<WRITE>: one lane per label follows the outer boundary of the label's first component crack by crack (two map reads per crack,
// each checked against the window, so no map and no extent can take it out of bounds; the number of cracks is capped by the lattice edges of
// the clamped box).  Nuclei are compact, so a lane's reads stay on a few neighbouring map rows that the L2 holds; a slide has 10^4 - 2.5 *
// 10^5 labels, so the launch is wide although each lane is serial.  The counting form leaves {V, twice the enclosed area, cracks, flags}; the
// writing form walks again and stores vertex k at row offsets[r] + k, every index checked against the label's range and the total.
//
// hull_kernel: one wave per label, no workgroup barrier (as in measure.hip).  Lanes are the columns of the box in chunks of 64: one ballot
// per row and chunk gives the row's leftmost and rightmost entry, GROUP rows' loads in flight at once.  Per lattice row y the leftmost and
// rightmost corner go into the wave's LDS; lanes 0 and 1 run one monotone-chain pass each (right chain downwards, left chain upwards, the
// stack in place over the points already read); then all lanes share the hull's edges: per edge the shoelace term, the length and the
// largest cross product over the corners (minimum Feret), per corner the largest squared distance to a later corner (maximum Feret), and a
// shuffle reduction.  All integers are exact (coordinates relative to the box, |cross| < 2^22).
// Measured (profiles/outline_ab.txt, profiles/outline_hull_ab.txt): at 2.5 * 10^5 labels the three launches take 0.45, 0.61
// and 0.65 ms beside 1.44 ms of hdy_label_measure on the same map; the hull is bound by the waves a CU holds, hence its two instances.
//
// Contract: no allocation, everything on the passed stream, no host synchronisation; all argument checks before any launch.
#include "label_common.h"
#include "hdyolo_outline.h"

namespace {

constexpr int MAX_SIDE = HDY_OUTLINE_MAX_SIDE;
constexpr int WALK_THREADS = 64;                 // a wave per workgroup: the walks of a wave end with its longest, so waves are spread over all CUs
constexpr int GROUP = 4;                         // map rows of a box whose loads are in flight together
// hull_kernel<LV, THREADS> takes the labels whose box has fewer than LV rows when LV is SMALL_LV, the others when it is BIG_LV: the wave's LDS
// (two chains of LV corners) is what bounds the waves per CU, and the pass is bound by the latency of a wave's dependent steps, so the waves
// per CU are its speed (measured); nuclei have tens of rows
constexpr int SMALL_LV = 128, SMALL_THREADS = 256;
constexpr int BIG_LV = MAX_SIDE + 1, BIG_THREADS = 64;
constexpr int MAX_BLOCKS = 1 << 16;
enum { FLAG_EXTENT = 4 };                       // beside FLAG_EMPTY and FLAG_SIDE: the extent was not this map's

// the pixel to the right of the crack that leaves corner (x, y) in direction d (0: +x, 1: +y, 2: -x, 3: -y; y points down), as (row, column)
// offsets from (y, x): right of +x is below, right of +y is to the left, right of -x is above, right of -y is to the right
__host__ __device__ __forceinline__ void right_of(int d, int& di, int& dj) {
    di = (d == 0 || d == 1) ? 0 : -1;
    dj = (d == 0 || d == 3) ? 0 : -1;
}

// the walk of one label; WRITE: true is returned when the label's range of offsets is not the one its walk fills.  Plain C++ on plain
// pointers, compiled for the host too, so that a stand-alone program can run it under a host sanitizer
template <bool WRITE>
__host__ __device__ __forceinline__ bool walk_label(const int* __restrict__ map, int h, int w, const int* __restrict__ extent, int r,
                                                    long long* __restrict__ counts, const long long* __restrict__ offsets,
                                                    int* __restrict__ verts, long long total) {
    const Box b = clamped_box(extent, r, h, w, MAX_SIDE);
    int flag = b.flag;
    long long V = 0, area2 = 0, L = 0;
    long long lo = 0, hi = 0;                                          // WRITE: the label's rows of verts are [lo, hi)
    if (WRITE) {
        lo = offsets[r];
        hi = offsets[r + 1];
        if (hi > total) hi = total;
        if (lo < 0) hi = lo;                                           // an offset below 0: nothing may be stored
    }
    if (!flag) {
        int j0 = -1;
        for (int j = b.x0; j < b.x0 + b.bw; ++j)
            if (map[(long long)b.y0 * w + j] == r) {                   // inside the window: the box is clamped
                j0 = j;
                break;
            }
        const int i0 = b.y0;
        if (j0 < 0 || owns(map, h, w, i0 - 1, j0, r) || owns(map, h, w, i0, j0 - 1, r)) flag = FLAG_EXTENT;
        if (!flag) {
            const long long cap = (long long)b.bw * (b.bh + 1) + (long long)b.bh * (b.bw + 1);
            int x = j0, y = i0, d = 0;
            bool closed = false;
            if (WRITE && lo < hi) {
                verts[2 * lo] = x;
                verts[2 * lo + 1] = y;
            }
            V = 1;
            for (long long step = 0; step < cap; ++step) {
                const int nx = x + (d == 0) - (d == 2), ny = y + (d == 1) - (d == 3);
                area2 += (long long)x * ny - (long long)nx * y;
                x = nx;
                y = ny;
                ++L;
                int ri, rj, li, lj;
                right_of(d, ri, rj);
                right_of((d + 3) & 3, li, lj);                         // left of d = right of the crack turned left
                int nd;
                if (!owns(map, h, w, y + ri, x + rj, r)) nd = (d + 1) & 3;
                else if (owns(map, h, w, y + li, x + lj, r)) nd = (d + 3) & 3;
                else nd = d;
                if (x == j0 && y == i0 && nd == 0) {
                    closed = true;
                    break;
                }
                if (nd != d) {
                    if (WRITE && lo + V < hi) {
                        verts[2 * (lo + V)] = x;
                        verts[2 * (lo + V) + 1] = y;
                    }
                    ++V;
                }
                d = nd;
            }
            if (!closed || area2 <= 0) flag = FLAG_EXTENT;
        }
    }
    if (flag) V = area2 = L = 0;
    if (WRITE) return (unsigned long long)offsets[r + 1] - (unsigned long long)offsets[r] != (unsigned long long)V || lo < 0 || offsets[r + 1] > total;
    long long* c = counts + 4 * (size_t)r;
    c[0] = V; c[1] = area2; c[2] = L; c[3] = flag;
    return false;
}

template <bool WRITE>
__global__ __launch_bounds__(WALK_THREADS) void walk_kernel(const int* __restrict__ map, int h, int w, const int* __restrict__ extent, int R,
                                                            long long* __restrict__ counts, const long long* __restrict__ offsets,
                                                            int* __restrict__ verts, long long total, int* __restrict__ status) {
    const long long stride = (long long)gridDim.x * WALK_THREADS;
    for (long long r = (long long)blockIdx.x * WALK_THREADS + threadIdx.x; r < R; r += stride)
        if (walk_label<WRITE>(map, h, w, extent, (int)r, counts, offsets, verts, total)) atomicOr(status, 1);
}

__global__ void clear_status_kernel(int* status) { *status = 0; }

__device__ __forceinline__ long long cross3(int ax, int ay, int bx, int by, int cx, int cy) {
    return (long long)(bx - ax) * (cy - by) - (long long)(by - ay) * (cx - bx);
}

template <int LV, int THREADS>
__global__ __launch_bounds__(THREADS) void hull_kernel(const int* __restrict__ map, int h, int w, const int* __restrict__ extent, int R,
                                                       long long* __restrict__ hull_i, double* __restrict__ hull_f) {
    constexpr int HULL_WAVES = THREADS / 64;
    // per wave and chain (0: right, top to bottom; 1: left, bottom to top) the corner per lattice row in the order the chain is walked,
    // x | y << 16 relative to the box, -1 where the label has no pixel beside the row; the hull's stack grows over the entries already read
    __shared__ int chain_s[HULL_WAVES][2][LV];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int* right = chain_s[wv][0];
    int* left = chain_s[wv][1];
    const long long waves = (long long)gridDim.x * HULL_WAVES;
    for (long long rr = (long long)blockIdx.x * HULL_WAVES + wv; rr < R; rr += waves) {      // wave-uniform
        const int r = (int)rr;
        const Box b = clamped_box(extent, r, h, w, MAX_SIDE);
        if ((b.bh < SMALL_LV) != (LV == SMALL_LV)) continue;           // the other instance's label (flagged labels have bh = 0 or are caught below)
        int flag = b.flag;
        int n0 = 0, n1 = 0;
        if (!flag) {
            // ---- the leftmost and rightmost entry of every row, GROUP rows at a time; the corner per lattice row
            int plo = MAX_SIDE + 1, phi = -1;                          // the row above: none
            for (int k0 = 0; k0 < b.bh; k0 += GROUP) {
                int lo[GROUP], hi[GROUP];
#pragma unroll
                for (int q = 0; q < GROUP; ++q) lo[q] = MAX_SIDE + 1, hi[q] = -1;
                for (int c0 = 0; c0 < b.bw; c0 += 64) {
                    const int c = c0 + lane;
                    int v[GROUP];
#pragma unroll
                    for (int q = 0; q < GROUP; ++q)
                        v[q] = (c < b.bw && k0 + q < b.bh) ? map[(long long)(b.y0 + k0 + q) * w + b.x0 + c] : -1;      // inside the clamped box
#pragma unroll
                    for (int q = 0; q < GROUP; ++q) {
                        const unsigned long long m = __ballot(v[q] == r);
                        if (m) {
                            if (lo[q] > MAX_SIDE) lo[q] = c0 + __ffsll(m) - 1;
                            hi[q] = c0 + 63 - __clzll((long long)m);
                        }
                    }
                }
#pragma unroll
                for (int q = 0; q < GROUP; ++q) {
                    const int k = k0 + q;
                    if (k < b.bh) {
                        if (k == 0 && hi[q] < 0) flag = FLAG_EXTENT;
                        const int l = plo < lo[q] ? plo : lo[q], g = phi > hi[q] ? phi : hi[q];
                        if (lane == 0) {
                            right[k] = g < 0 ? -1 : (g + 1) | k << 16;
                            left[b.bh - k] = g < 0 ? -1 : l | k << 16;
                        }
                        plo = lo[q];
                        phi = hi[q];
                    }
                }
                if (flag) break;                                       // wave-uniform: set from a ballot
            }
            if (lane == 0) {
                right[b.bh] = phi < 0 ? -1 : (phi + 1) | b.bh << 16;
                left[0] = phi < 0 ? -1 : plo | b.bh << 16;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        if (!flag) {
            // ---- two monotone-chain passes, lane 0 the right chain and lane 1 the left one; a turn is convex when the cross product is > 0
            int n = 0;
            if (lane < 2) {
                int* p = lane ? left : right;
                for (int t = 0; t <= b.bh; ++t) {
                    const int c = p[t];
                    if (c < 0) continue;
                    const int cx = c & 0xFFFF, cy = c >> 16;
                    while (n >= 2) {
                        const int a = p[n - 2], m = p[n - 1];
                        if (cross3(a & 0xFFFF, a >> 16, m & 0xFFFF, m >> 16, cx, cy) > 0) break;
                        --n;
                    }
                    p[n++] = c;                                        // n <= t: the stack never passes the read position
                }
            }
            n0 = __shfl(n, 0);
            n1 = __shfl(n, 1);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        const int H = n0 + n1;                                         // 0 for a flagged label
        long long area2 = 0, fmax2 = 0;
        double perim = 0.0, fmin = 1e300;
        for (int e = lane; e < H; e += 64) {
            const int a = e < n0 ? right[e] : left[e - n0];
            const int e1 = e + 1 == H ? 0 : e + 1;
            const int c = e1 < n0 ? right[e1] : left[e1 - n0];
            const int ax = a & 0xFFFF, ay = a >> 16, cx = c & 0xFFFF, cy = c >> 16;
            // the shoelace term about the box's corner: a translation does not change the closed sum
            area2 += (long long)ax * cy - (long long)cx * ay;
            const long long len2 = (long long)(cx - ax) * (cx - ax) + (long long)(cy - ay) * (cy - ay);
            const double len = sqrt((double)len2);
            perim += len;
            long long far = 0;
            for (int v = 0; v < H; ++v) {
                const int p = v < n0 ? right[v] : left[v - n0];
                const int px = p & 0xFFFF, py = p >> 16;
                const long long cr = cross3(ax, ay, cx, cy, px, py);   // >= 0: every corner lies on the hull's inner side of the edge
                if (cr > far) far = cr;
                if (v > e) {
                    const long long d2 = (long long)(px - ax) * (px - ax) + (long long)(py - ay) * (py - ay);
                    if (d2 > fmax2) fmax2 = d2;
                }
            }
            const double width = (double)far / len;
            if (width < fmin) fmin = width;
        }
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {                           // a fixed tree: the sums do not depend on anything but the inputs
            area2 += __shfl_xor(area2, s);
            perim += __shfl_xor(perim, s);
            const long long om = __shfl_xor(fmax2, s);
            fmax2 = om > fmax2 ? om : fmax2;
            const double of = __shfl_xor(fmin, s);
            fmin = of < fmin ? of : fmin;
        }
        if (lane == 0) {
            long long* o = hull_i + 4 * (size_t)r;
            o[0] = H; o[1] = area2; o[2] = fmax2; o[3] = flag;
            hull_f[2 * (size_t)r] = H ? perim : 0.0;
            hull_f[2 * (size_t)r + 1] = H ? fmin : 0.0;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");         // the chains are read before the next label overwrites them
        __builtin_amdgcn_wave_barrier();
    }
}

// what the three entry points read: the map window, the extent table and their two pointers
int check_inputs(const char* who, const int* map, long long map_elems, int h, int w, const int* extent, long long extent_elems, int R) {
    HDY_CHECKED(check_map(who, map_elems, h, w, HDY_OUTLINE_MAX_WINDOW));
    HDY_CHECKED(check_extent(who, extent_elems, R, "reads"));
    HDY_ARG(R == 0 || (map && extent), "%s: null map or extent pointer", who);
    HDY_ARG((((uintptr_t)map | (uintptr_t)extent) & 3) == 0, "%s: misaligned pointer (map, extent 4 bytes)", who);
    return HDY_OK;
}

}  // namespace

extern "C" {

int hdy_outline_revision(void) { return HDY_OUTLINE_REVISION; }

int hdy_label_outline_count(const int* map, long long map_elems, int h, int w, const int* extent, long long extent_elems, int R,
                            long long* counts, long long counts_elems, void* stream) {
    const char* who = "label_outline_count";
    HDY_ARG(counts_elems >= 0, "%s: negative count (counts_elems=%lld)", who, counts_elems);
    HDY_CHECKED(check_inputs(who, map, map_elems, h, w, extent, extent_elems, R));
    HDY_ARG(counts_elems == 4ll * R, "%s: counts_elems=%lld, the call writes 4 * R = 4 * %d", who, counts_elems, R);
    HDY_ARG(R == 0 || counts, "%s: null counts pointer", who);
    HDY_ARG(((uintptr_t)counts & 7) == 0, "%s: misaligned pointer (counts 8 bytes)", who);
    if (R == 0) return HDY_OK;
    hipLaunchKernelGGL(walk_kernel<false>, dim3(label_blocks(R, WALK_THREADS, MAX_BLOCKS)), dim3(WALK_THREADS), 0, (hipStream_t)stream, map, h, w, extent, R, counts,
                       (const long long*)nullptr, (int*)nullptr, 0ll, (int*)nullptr);
    HDY_LAUNCH_CHECK(who);
    hdy_note_dispatch("label_outline_count");
    return HDY_OK;
}

int hdy_label_outline_write(const int* map, long long map_elems, int h, int w, const int* extent, long long extent_elems, int R,
                            const long long* offsets, long long offsets_elems, int* verts, long long verts_elems, int* status, void* stream) {
    const char* who = "label_outline_write";
    HDY_ARG(offsets_elems >= 0 && verts_elems >= 0, "%s: negative count (offsets_elems=%lld, verts_elems=%lld)", who, offsets_elems, verts_elems);
    HDY_CHECKED(check_inputs(who, map, map_elems, h, w, extent, extent_elems, R));
    HDY_ARG(offsets_elems == (long long)R + 1, "%s: offsets_elems=%lld, the call reads R + 1 = %d + 1", who, offsets_elems, R);
    HDY_ARG((verts_elems & 1) == 0, "%s: verts_elems=%lld is odd, a vertex is two entries", who, verts_elems);
    HDY_ARG(R == 0 || (offsets && status && (verts || verts_elems == 0)), "%s: null offsets, verts or status pointer", who);
    HDY_ARG(((uintptr_t)offsets & 7) == 0 && (((uintptr_t)verts | (uintptr_t)status) & 3) == 0,
            "%s: misaligned pointer (offsets 8 bytes; verts, status 4 bytes)", who);
    if (R == 0) return HDY_OK;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(clear_status_kernel, dim3(1), dim3(1), 0, st, status);
    hipLaunchKernelGGL(walk_kernel<true>, dim3(label_blocks(R, WALK_THREADS, MAX_BLOCKS)), dim3(WALK_THREADS), 0, st, map, h, w, extent, R, (long long*)nullptr, offsets,
                       verts, verts_elems / 2, status);
    HDY_LAUNCH_CHECK(who);
    hdy_note_dispatch("label_outline_write");
    return HDY_OK;
}

int hdy_label_hull(const int* map, long long map_elems, int h, int w, const int* extent, long long extent_elems, int R, long long* hull_i,
                   long long hull_i_elems, double* hull_f, long long hull_f_elems, void* stream) {
    const char* who = "label_hull";
    HDY_ARG(hull_i_elems >= 0 && hull_f_elems >= 0, "%s: negative count (hull_i_elems=%lld, hull_f_elems=%lld)", who, hull_i_elems, hull_f_elems);
    HDY_CHECKED(check_inputs(who, map, map_elems, h, w, extent, extent_elems, R));
    HDY_ARG(hull_i_elems == 4ll * R, "%s: hull_i_elems=%lld, the call writes 4 * R = 4 * %d", who, hull_i_elems, R);
    HDY_ARG(hull_f_elems == 2ll * R, "%s: hull_f_elems=%lld, the call writes 2 * R = 2 * %d", who, hull_f_elems, R);
    HDY_ARG(R == 0 || (hull_i && hull_f), "%s: null hull_i or hull_f pointer", who);
    HDY_ARG((((uintptr_t)hull_i | (uintptr_t)hull_f) & 7) == 0, "%s: misaligned pointer (hull_i, hull_f 8 bytes)", who);
    if (R == 0) return HDY_OK;
    hipLaunchKernelGGL((hull_kernel<SMALL_LV, SMALL_THREADS>), dim3(label_blocks(R, SMALL_THREADS / 64, MAX_BLOCKS)), dim3(SMALL_THREADS), 0,
                       (hipStream_t)stream, map, h, w, extent, R, hull_i, hull_f);
    hipLaunchKernelGGL((hull_kernel<BIG_LV, BIG_THREADS>), dim3(label_blocks(R, BIG_THREADS / 64, MAX_BLOCKS)), dim3(BIG_THREADS), 0,
                       (hipStream_t)stream, map, h, w, extent, R, hull_i, hull_f);
    HDY_LAUNCH_CHECK(who);
    hdy_note_dispatch("label_hull");
    return HDY_OK;
}

}  // extern "C"
