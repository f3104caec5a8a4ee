// Neighbourhood features of a slide's nuclei (hdy_spatial_cells, hdy_spatial_neighbors, hdy_spatial_density): a binned neighbour search over
// points in units of 1/16 pixel.  All integer; bound by loads and LDS, no MFMA, no LDS-DMA, no float anywhere.
//
// The arithmetic is stated in include/hdyolo_spatial.h and restated in tests/spatial_ref.py.
//
// cells_kernel: pts arrives sorted by cell (row-major cells, absent points last).  One lane per cell c, c = 0 .. ncells: cell_start[c] is the
// lower bound of c among the sorted cells, by bisection over pts (log2 N 16-byte loads, the upper levels of the search shared by every lane).
// That costs more loads than a head-of-run scatter but needs no second pass for the empty cells, bounds every lane's work by log2 N whatever
// the point set, and leaves every entry inside [0, N] on any content.  The same lanes, one per point, compare each point's cell with its
// predecessor's and OR bit 0 into the status word (an integer atomic, issued only on a violation).
//
// neighbors_kernel: one lane per sorted position, `threads` consecutive positions per workgroup: neighbouring lanes query from the same or the
// next cell, so a wave walks nearly the same candidates and its loads meet in the cache.  The nine cells around a query are three runs of
// three consecutive cells (row-major order), clipped at the grid's edges: three contiguous ranges of pts, each from two entries of cell_start,
// a candidate per 16-byte load.  A candidate within r_K increments ONE ring counter (the smallest k with d2 <= r_k^2; the counts are made
// cumulative before the store) and is compared with the class's nearest record (d2, then original row).  The K * C ring counters and C nearest
// records are indexed by a run-time class, so they live in LDS laid out [slot][lane] (conflict-free, no scratch memory), never in a
// dynamically indexed register array; the lane owns its column, so there is no barrier and no atomic.  The workgroup is 256 lanes while the
// slots fit 64 KB and 128 beyond (K * C + 3 C <= 112 words per lane).  A cell may hold every point: a lane does (points in its nine cells)
// tests, nothing assumes a bound per cell.  The form that stages the union of a workgroup's ranges in LDS was not built.
//
// density_kernel: one lane per point, one integer atomicAdd into the field's class counter; the grid is zeroed by a pass of the same call.
//
// Contract: no allocation, everything on the passed stream, no host synchronisation; all argument checks before any launch.
#include "spatial_common.h"

namespace {

typedef unsigned long long u64;

constexpr int THREADS = 256;
constexpr int MAXC = HDY_SPATIAL_MAX_CLASSES, MAXK = HDY_SPATIAL_MAX_RADII;
constexpr int LDS_BUDGET = 64 * 1024;
static_assert((MAXK * MAXC + 3 * MAXC) * 128 * 4 <= LDS_BUDGET, "the slots of 128 lanes fit the static LDS budget at the limits");

__global__ __launch_bounds__(THREADS) void cells_kernel(const i32x4* __restrict__ pts, int N, Grid g, int* __restrict__ cell_start,
                                                        int* __restrict__ status) {
    const long long t = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (t <= g.ncells) {                                      // lower bound of cell t among the sorted cells
        int lo = 0, hi = N;
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if (cell_of(pts[mid], g) < (int)t) lo = mid + 1; else hi = mid;
        }
        cell_start[t] = lo;
    }
    if (t >= 1 && t < N && cell_of(pts[t], g) < cell_of(pts[t - 1], g)) atomicOr(status, 1);
}

struct NArgs {
    const i32x4* pts;
    const int* cell_start;
    int N, K, C;
    Grid g;
    long long r2[MAXK];
    int* counts;
    long long* near_d2;
    int* near_row;
};

__global__ __launch_bounds__(THREADS) void neighbors_kernel(const NArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int T = blockDim.x, lane = threadIdx.x, K = a.K, C = a.C;
    // [C][T] nearest d2 (8 bytes), [C][T] nearest row, [K * C][T] ring counters: the lane's column of every slot is its own
    u64* best = (u64*)smem;
    int* brow = (int*)(best + (size_t)C * T);
    int* ring = brow + (size_t)C * T;
    const long long i = (long long)blockIdx.x * T + lane;
    if (i >= a.N) return;
    const i32x4 me = a.pts[i];
    const bool row_ok = (unsigned)me.w < (unsigned)a.N;
    const size_t row = (size_t)(row_ok ? me.w : 0);
    if (me.x < 0 || me.y < 0) {                              // absent: zeros and -1
        if (row_ok) {
            for (int s = 0; s < K * C; ++s) a.counts[row * K * C + s] = 0;
            for (int c = 0; c < C; ++c) {
                a.near_d2[row * C + c] = -1;
                a.near_row[row * C + c] = -1;
            }
        }
        return;
    }
    for (int c = 0; c < C; ++c) {
        best[c * T + lane] = ~0ull;
        brow[c * T + lane] = 0x7fffffff;
    }
    for (int s = 0; s < K * C; ++s) ring[s * T + lane] = 0;
    const long long r2a = a.r2[0], r2b = a.r2[1], r2c = a.r2[2], rmax2 = a.r2[MAXK - 1];
    static_assert(MAXK == 4, "ring selection");
    const int cx = min(me.x / a.g.cell, a.g.ncx - 1), cy = min(me.y / a.g.cell, a.g.ncy - 1);
    const int c0 = max(cx - 1, 0), c1 = min(cx + 1, a.g.ncx - 1);
    for (int ry = max(cy - 1, 0); ry <= min(cy + 1, a.g.ncy - 1); ++ry) {
        const Run span = cell_run(a.cell_start, a.g, a.N, ry, c0, c1);     // three consecutive cells of one grid row
        for (int j = span.s; j < span.e; ++j) {
            const i32x4 q = a.pts[j];
            const long long dx = (long long)q.x - me.x, dy = (long long)q.y - me.y;
            const long long d2 = dx * dx + dy * dy;
            // another point (identity: the sorted position), present, of a counted class, within the largest radius
            if (j == (int)i || q.x < 0 || q.y < 0 || (unsigned)q.z >= (unsigned)C || d2 > rmax2) continue;
            const int k = (d2 > r2a) + (d2 > r2b) + (d2 > r2c);      // the smallest k with d2 <= r_k^2 (< K: the entries from K - 1 on hold r_K^2)
            ring[(k * C + q.z) * T + lane] += 1;
            const u64 b = best[q.z * T + lane];
            if ((u64)d2 < b || ((u64)d2 == b && q.w < brow[q.z * T + lane])) {
                best[q.z * T + lane] = (u64)d2;
                brow[q.z * T + lane] = q.w;
            }
        }
    }
    if (!row_ok) return;
    for (int c = 0; c < C; ++c) {
        int run = 0;
        for (int k = 0; k < K; ++k) {                        // rings -> cumulative counts
            run += ring[(k * C + c) * T + lane];
            a.counts[(row * K + k) * C + c] = run;
        }
        const u64 b = best[c * T + lane];
        a.near_d2[row * C + c] = b == ~0ull ? -1ll : (long long)b;
        a.near_row[row * C + c] = b == ~0ull ? -1 : brow[c * T + lane];
    }
}

__global__ __launch_bounds__(THREADS) void zero_kernel(int* __restrict__ p, long long n) {
    const long long stride = (long long)gridDim.x * THREADS;
    for (long long i = (long long)blockIdx.x * THREADS + threadIdx.x; i < n; i += stride) p[i] = 0;
}

__global__ __launch_bounds__(THREADS) void density_kernel(const i32x4* __restrict__ pts, int N, int g_units, int gx, int gy, int C,
                                                          int* __restrict__ grid) {
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (i >= N) return;
    const i32x4 p = pts[i];
    if (p.x < 0 || p.y < 0 || (unsigned)p.z >= (unsigned)C) return;
    const int fx = p.x / g_units, fy = p.y / g_units;
    if (fx >= gx || fy >= gy) return;
    atomicAdd(&grid[((size_t)fy * gx + fx) * C + p.z], 1);
}

}  // namespace

extern "C" {

int hdy_spatial_revision(void) { return HDY_SPATIAL_REVISION; }

int hdy_spatial_cells(const int* pts, long long pts_elems, int N, int cell_units, int ncx, int ncy, int* cell_start, long long cell_start_elems,
                      int* status, long long status_elems, void* stream) {
    const char* who = "spatial_cells";
    HDY_CHECKED(check_pts(who, pts, pts_elems, N));
    HDY_CHECKED(check_grid(who, cell_units, ncx, ncy));
    const int ncells = ncx * ncy;
    HDY_CHECKED(check_cell_start(who, cell_start_elems, ncells, "writes"));
    HDY_ARG(status_elems == 1, "%s: status_elems=%lld, the call writes 1", who, status_elems);
    HDY_ARG(N == 0 || (cell_start && status), "%s: null cell_start or status pointer", who);
    HDY_ARG((((uintptr_t)cell_start | (uintptr_t)status) & 3) == 0, "%s: misaligned pointer (cell_start, status 4 bytes)", who);
    if (N == 0) return HDY_OK;
    hipStream_t st = (hipStream_t)stream;
    HDY_CHECKED(hdy_memset_async(who, status, 0, sizeof(int), st));
    const Grid g = {cell_units, ncx, ncy, ncells};
    const long long items = (long long)ncells + 1 > N ? (long long)ncells + 1 : N;
    hipLaunchKernelGGL(cells_kernel, dim3((unsigned)((items + THREADS - 1) / THREADS)), dim3(THREADS), 0, st, (const i32x4*)pts, N, g, cell_start, status);
    HDY_LAUNCH_CHECK(who);
    hdy_note_dispatch("spatial_cells");
    return HDY_OK;
}

int hdy_spatial_neighbors(const int* pts, long long pts_elems, int N, const int* cell_start, long long cell_start_elems, int cell_units, int ncx,
                          int ncy, const int* radii, int K, int C, int* counts, long long counts_elems, long long* near_d2, long long near_d2_elems,
                          int* near_row, long long near_row_elems, void* stream) {
    const char* who = "spatial_neighbors";
    HDY_CHECKED(check_pts(who, pts, pts_elems, N));
    HDY_CHECKED(check_grid(who, cell_units, ncx, ncy));
    HDY_ARG(C >= 1 && C <= MAXC, "%s: C=%d outside [1, %d]", who, C, MAXC);
    HDY_ARG(K >= 1 && K <= MAXK, "%s: K=%d outside [1, %d]", who, K, MAXK);
    HDY_ARG(radii, "%s: null radii pointer (a host array of K radii)", who);
    HDY_ARG(((uintptr_t)radii & 3) == 0, "%s: misaligned pointer (radii 4 bytes)", who);
    for (int k = 0; k < K; ++k)
        HDY_ARG(radii[k] >= 1 && (k == 0 || radii[k] > radii[k - 1]), "%s: radii must increase strictly from 1 (radii[%d]=%d)", who, k, radii[k]);
    HDY_ARG(radii[K - 1] <= cell_units, "%s: the largest radius %d passes cell_units=%d", who, radii[K - 1], cell_units);
    const int ncells = ncx * ncy;
    HDY_CHECKED(check_cell_start(who, cell_start_elems, ncells, "reads"));
    HDY_ARG(counts_elems == (long long)N * K * C, "%s: counts_elems=%lld, the call writes N * K * C = %d * %d * %d", who, counts_elems, N, K, C);
    HDY_ARG(near_d2_elems == (long long)N * C, "%s: near_d2_elems=%lld, the call writes N * C = %d * %d", who, near_d2_elems, N, C);
    HDY_ARG(near_row_elems == (long long)N * C, "%s: near_row_elems=%lld, the call writes N * C = %d * %d", who, near_row_elems, N, C);
    HDY_ARG(N == 0 || (cell_start && counts && near_d2 && near_row), "%s: null cell_start, counts, near_d2 or near_row pointer", who);
    HDY_ARG(((uintptr_t)near_d2 & 7) == 0 && (((uintptr_t)cell_start | (uintptr_t)counts | (uintptr_t)near_row) & 3) == 0,
            "%s: misaligned pointer (near_d2 8 bytes; cell_start, counts, near_row 4 bytes)", who);
    if (N == 0) return HDY_OK;
    NArgs a = {};
    a.pts = (const i32x4*)pts; a.cell_start = cell_start; a.N = N; a.K = K; a.C = C;
    a.g = {cell_units, ncx, ncy, ncells};
    for (int k = 0; k < MAXK; ++k) a.r2[k] = (long long)radii[k < K ? k : K - 1] * radii[k < K ? k : K - 1];
    a.counts = counts; a.near_d2 = near_d2; a.near_row = near_row;
    const int words = K * C + 3 * C;                                         // LDS words per lane
    const int threads = words * THREADS * 4 <= LDS_BUDGET ? THREADS : THREADS / 2;
    hipLaunchKernelGGL(neighbors_kernel, dim3((unsigned)(((long long)N + threads - 1) / threads)), dim3(threads), (size_t)words * threads * 4,
                       (hipStream_t)stream, a);
    HDY_LAUNCH_CHECK(who);
    hdy_note_dispatch("spatial_neighbors");
    return HDY_OK;
}

int hdy_spatial_density(const int* pts, long long pts_elems, int N, int g_units, int gx, int gy, int C, int* grid, long long grid_elems,
                        void* stream) {
    const char* who = "spatial_density";
    HDY_CHECKED(check_pts(who, pts, pts_elems, N));
    HDY_ARG(C >= 1 && C <= MAXC, "%s: C=%d outside [1, %d]", who, C, MAXC);
    HDY_ARG(g_units >= 1, "%s: g_units=%d must be positive", who, g_units);
    HDY_ARG(gx >= 1 && gy >= 1 && (long long)gx * gy * C < (1ll << 31), "%s: a grid of %d x %d fields of %d classes (sides >= 1, fewer than 2^31 entries)",
            who, gx, gy, C);
    HDY_ARG(grid_elems == (long long)gx * gy * C, "%s: grid_elems=%lld, the call writes gy * gx * C = %d * %d * %d", who, grid_elems, gy, gx, C);
    HDY_ARG(N == 0 || grid, "%s: null grid pointer", who);
    HDY_ARG(((uintptr_t)grid & 3) == 0, "%s: misaligned pointer (grid 4 bytes)", who);
    if (N == 0) return HDY_OK;
    hipStream_t st = (hipStream_t)stream;
    const long long zero_blocks = (grid_elems + THREADS - 1) / THREADS;
    hipLaunchKernelGGL(zero_kernel, dim3((unsigned)(zero_blocks < 4096 ? zero_blocks : 4096)), dim3(THREADS), 0, st, grid, grid_elems);
    hipLaunchKernelGGL(density_kernel, dim3((unsigned)(((long long)N + THREADS - 1) / THREADS)), dim3(THREADS), 0, st, (const i32x4*)pts, N, g_units, gx,
                       gy, C, grid);
    HDY_LAUNCH_CHECK(who);
    hdy_note_dispatch("spatial_density");
    return HDY_OK;
}

}  // extern "C"
