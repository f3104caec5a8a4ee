// The cell graph of a slide's nuclei (hdy_graph_knn, hdy_graph_mutual): the k nearest neighbours of every point by an adaptive ring search over
// the cells of csrc/spatial.hip, and which of those edges are mutual.  All integer; bound by loads and LDS, no MFMA, no float anywhere.
//
// The arithmetic, the stop rule and its proof are stated in include/hdyolo_graph.h and restated in tests/graph_ref.py.
//
// knn_kernel: one lane per sorted position, as neighbors_kernel of spatial.hip: neighbouring lanes query from the same or the next cell, so a
// wave walks nearly the same candidates and its loads meet in the cache.  Ring t around the lane's cell is the cells at Chebyshev distance t:
// its two outer grid rows are one contiguous range of pts each (two entries of cell_start), the rows between give the two single cells at
// columns cx - t and cx + t.  Everything is clipped at the grid and clamped into [0, N].  After a ring the lane tests the stop rule; lanes of
// one wave stop at different rings (a dense cluster beside sparse points), the wave runs until its last lane stops.  The last ring is at most
// `rings` = ceil(max_radius / cell_units) <= HDY_GRAPH_MAX_RINGS, checked on the host.
//
// The lane's k best (d2, row) records, ascending, are indexed at run time, so they live in LDS laid out [slot][lane] (conflict-free, no
// scratch memory), never in a dynamically indexed register array: 12 * k bytes per lane, 48 KB for 256 lanes at k = 16.  The lane owns its
// column: no barrier, no atomic.  The worst kept record is mirrored in registers: a candidate is compared with it first and touches LDS only
// when it is better (or the list is not full yet); then it is inserted by shifting the records behind it one slot down, at most k - 1 moves.
//
// mutual_kernel: one lane per (p, s): k loads of the row of q = nbr_row[p][s].
//
// Contract: no allocation, everything on the passed stream, no host synchronisation; all argument checks before any launch.
#include "hdyolo_graph.h"
#include "spatial_common.h"

namespace {

typedef unsigned long long u64;

constexpr int THREADS = 256;
constexpr int MAXK = HDY_GRAPH_MAX_K, MAXRINGS = HDY_GRAPH_MAX_RINGS;
static_assert(MAXK * 12 * THREADS <= 64 * 1024, "the lists of a workgroup fit the static LDS budget at the limit");

struct KArgs {
    const i32x4* pts;
    const int* cell_start;
    int N, k, rings;
    Grid g;
    long long rmax, rmax2;
    int* nbr_row;
    long long* nbr_d2;
    int* nbr_count;
};

// the lane's list: ld2 / lrow [k][T], n records held, (wd2, wrow) = the record in slot k - 1 once n == k
struct List {
    u64* d2;
    int* row;
    int T, lane, k, n;
    u64 wd2;
    int wrow;
};

__device__ __forceinline__ void offer(List& l, u64 d2, int row) {
    if (l.n == l.k && (d2 > l.wd2 || (d2 == l.wd2 && row >= l.wrow))) return;        // not better than the worst kept record
    int s = l.n < l.k ? l.n : l.k - 1;                                               // the slot that opens: the end, or the worst record's
    while (s > 0) {                                                                   // at most k - 1 moves
        const u64 pd = l.d2[(s - 1) * l.T + l.lane];
        const int pr = l.row[(s - 1) * l.T + l.lane];
        if (pd < d2 || (pd == d2 && pr < row)) break;
        l.d2[s * l.T + l.lane] = pd;
        l.row[s * l.T + l.lane] = pr;
        --s;
    }
    l.d2[s * l.T + l.lane] = d2;
    l.row[s * l.T + l.lane] = row;
    if (l.n < l.k) ++l.n;
    if (l.n == l.k) {
        l.wd2 = l.d2[(l.k - 1) * l.T + l.lane];
        l.wrow = l.row[(l.k - 1) * l.T + l.lane];
    }
}

// the candidates of the cells c0 .. c1 of grid row ry: one contiguous range of pts
__device__ __forceinline__ void scan(const KArgs& a, List& l, const i32x4& me, int self, int ry, int c0, int c1) {
    const Run span = cell_run(a.cell_start, a.g, a.N, ry, c0, c1);
    for (int j = span.s; j < span.e; ++j) {
        const i32x4 q = a.pts[j];
        if (j == self || q.x < 0 || q.y < 0 || q.z < 0) continue;                    // another point (identity), present, a node
        const long long dx = (long long)q.x - me.x, dy = (long long)q.y - me.y;
        const long long d2 = dx * dx + dy * dy;
        if (d2 <= a.rmax2) offer(l, (u64)d2, q.w);
    }
}

__global__ __launch_bounds__(THREADS) void knn_kernel(const KArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    List l;
    l.T = blockDim.x; l.lane = threadIdx.x; l.k = a.k; l.n = 0; l.wd2 = ~0ull; l.wrow = 0x7fffffff;
    l.d2 = (u64*)smem;
    l.row = (int*)(l.d2 + (size_t)a.k * l.T);
    const long long i = (long long)blockIdx.x * l.T + l.lane;
    if (i >= a.N) return;
    const i32x4 me = a.pts[i];
    const bool row_ok = (unsigned)me.w < (unsigned)a.N;
    const size_t row = (size_t)(row_ok ? me.w : 0);
    if (me.x >= 0 && me.y >= 0) {
        const int cx = min(me.x / a.g.cell, a.g.ncx - 1), cy = min(me.y / a.g.cell, a.g.ncy - 1);
        for (int t = 0; t <= a.rings; ++t) {
            const int x0 = max(cx - t, 0), x1 = min(cx + t, a.g.ncx - 1);
            if (cy - t >= 0) scan(a, l, me, (int)i, cy - t, x0, x1);
            if (t > 0 && cy + t <= a.g.ncy - 1) scan(a, l, me, (int)i, cy + t, x0, x1);
            for (int ry = max(cy - t + 1, 0); ry <= min(cy + t - 1, a.g.ncy - 1); ++ry) {  // at most 2 * rings - 1 rows
                if (cx - t >= 0) scan(a, l, me, (int)i, ry, cx - t, cx - t);
                if (cx + t <= a.g.ncx - 1) scan(a, l, me, (int)i, ry, cx + t, cx + t);
            }
            const long long reach = (long long)t * a.g.cell;                             // every unvisited point is further than this
            if (reach >= a.rmax) break;
            if (l.n == l.k && l.wd2 <= (u64)(reach * reach)) break;                      // reach < max_radius < 2^31: no overflow
            if (cx - t <= 0 && cx + t >= a.g.ncx - 1 && cy - t <= 0 && cy + t >= a.g.ncy - 1) break;
        }
    }
    if (!row_ok) return;
    for (int s = 0; s < a.k; ++s) {
        const bool held = s < l.n;
        a.nbr_row[row * a.k + s] = held ? l.row[s * l.T + l.lane] : -1;
        a.nbr_d2[row * a.k + s] = held ? (long long)l.d2[s * l.T + l.lane] : -1ll;
    }
    a.nbr_count[row] = l.n;
}

__global__ __launch_bounds__(THREADS) void mutual_kernel(const int* __restrict__ nbr_row, int N, int k, int* __restrict__ mutual) {
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (i >= (long long)N * k) return;
    const int p = (int)(i / k), q = nbr_row[i];
    int hit = 0;
    if ((unsigned)q < (unsigned)N)
        for (int s = 0; s < k; ++s) hit |= nbr_row[(long long)q * k + s] == p;
    mutual[i] = hit;
}

}  // namespace

extern "C" {

int hdy_graph_revision(void) { return HDY_GRAPH_REVISION; }

int hdy_graph_knn(const int* pts, long long pts_elems, int N, const int* cell_start, long long cell_start_elems, int cell_units, int ncx, int ncy,
                  int k, int max_radius, int* nbr_row, long long nbr_row_elems, long long* nbr_d2, long long nbr_d2_elems, int* nbr_count,
                  long long nbr_count_elems, void* stream) {
    const char* who = "graph_knn";
    HDY_CHECKED(check_pts(who, pts, pts_elems, N));
    HDY_CHECKED(check_grid(who, cell_units, ncx, ncy));
    HDY_ARG(k >= 1 && k <= MAXK, "%s: k=%d outside [1, %d]", who, k, MAXK);
    HDY_ARG(max_radius >= 1, "%s: max_radius=%d must be positive", who, max_radius);
    const long long rings = ((long long)max_radius + cell_units - 1) / cell_units;
    HDY_ARG(rings <= MAXRINGS, "%s: max_radius=%d is %lld rings of cell_units=%d, at most %d", who, max_radius, rings, cell_units, MAXRINGS);
    const int ncells = ncx * ncy;
    HDY_CHECKED(check_cell_start(who, cell_start_elems, ncells, "reads"));
    HDY_ARG(nbr_row_elems == (long long)N * k, "%s: nbr_row_elems=%lld, the call writes N * k = %d * %d", who, nbr_row_elems, N, k);
    HDY_ARG(nbr_d2_elems == (long long)N * k, "%s: nbr_d2_elems=%lld, the call writes N * k = %d * %d", who, nbr_d2_elems, N, k);
    HDY_ARG(nbr_count_elems == (long long)N, "%s: nbr_count_elems=%lld, the call writes N = %d", who, nbr_count_elems, N);
    HDY_ARG(N == 0 || (cell_start && nbr_row && nbr_d2 && nbr_count), "%s: null cell_start, nbr_row, nbr_d2 or nbr_count pointer", who);
    HDY_ARG(((uintptr_t)nbr_d2 & 7) == 0 && (((uintptr_t)cell_start | (uintptr_t)nbr_row | (uintptr_t)nbr_count) & 3) == 0,
            "%s: misaligned pointer (nbr_d2 8 bytes; cell_start, nbr_row, nbr_count 4 bytes)", who);
    if (N == 0) return HDY_OK;
    KArgs a = {};
    a.pts = (const i32x4*)pts; a.cell_start = cell_start; a.N = N; a.k = k;
    a.g = {cell_units, ncx, ncy, ncells}; a.rings = (int)rings;
    a.rmax = max_radius; a.rmax2 = (long long)max_radius * max_radius;
    a.nbr_row = nbr_row; a.nbr_d2 = nbr_d2; a.nbr_count = nbr_count;
    hipLaunchKernelGGL(knn_kernel, dim3((unsigned)(((long long)N + THREADS - 1) / THREADS)), dim3(THREADS), (size_t)k * 12 * THREADS,
                       (hipStream_t)stream, a);
    HDY_LAUNCH_CHECK(who);
    hdy_note_dispatch("graph_knn");
    return HDY_OK;
}

int hdy_graph_mutual(const int* nbr_row, long long nbr_row_elems, int N, int k, int* mutual, long long mutual_elems, void* stream) {
    const char* who = "graph_mutual";
    HDY_ARG(N >= 0, "%s: negative count (N=%d)", who, N);
    HDY_ARG(k >= 1 && k <= MAXK, "%s: k=%d outside [1, %d]", who, k, MAXK);
    HDY_ARG(nbr_row_elems == (long long)N * k, "%s: nbr_row_elems=%lld, the call reads N * k = %d * %d", who, nbr_row_elems, N, k);
    HDY_ARG(mutual_elems == (long long)N * k, "%s: mutual_elems=%lld, the call writes N * k = %d * %d", who, mutual_elems, N, k);
    HDY_ARG(N == 0 || (nbr_row && mutual), "%s: null nbr_row or mutual pointer", who);
    HDY_ARG((((uintptr_t)nbr_row | (uintptr_t)mutual) & 3) == 0, "%s: misaligned pointer (nbr_row, mutual 4 bytes)", who);
    if (N == 0) return HDY_OK;
    const long long items = (long long)N * k;
    hipLaunchKernelGGL(mutual_kernel, dim3((unsigned)((items + THREADS - 1) / THREADS)), dim3(THREADS), 0, (hipStream_t)stream, nbr_row, N, k, mutual);
    HDY_LAUNCH_CHECK(who);
    hdy_note_dispatch("graph_mutual");
    return HDY_OK;
}

}  // extern "C"
