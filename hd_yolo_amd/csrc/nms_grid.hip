// Exact greedy NMS of ONE large set of explicit boxes over the whole chip (hdy_nms_grid_begin / _round / _finish), bit-identical to
// detect.hip's nms_kernel (hdy_nms_boxes, one workgroup per set).  Scalar integer / fp32 work bound by latency and L2; no MFMA, no LDS-DMA.
//
// Rank r of a box = position of its key (desc_key(score) << 32 | row) in ascending order.  Box i is kept iff no KEPT box of higher rank
// (smaller r) has iou_gt with it; that recursion has one solution, and rounds over a three-valued state reach it:
//   an undecided box looks at its higher-ranked overlapping neighbours: one kept -> suppressed; none kept and none undecided -> kept; else wait.
// States only move from undecided to a final value, so a stale read delays a decision and never changes it: one launch per round, no
// grid barrier, no flag protocol.  The highest-ranked undecided box is decided in every round.
//
// Neighbours: iou_gt can only hold when the clamped intersection is positive, i.e. both boxes are proper (x2 > x1, y2 > y1) and their
// extents overlap.  Improper boxes are kept at once.  Proper boxes are binned by centre into a hierarchy of uniform grids: level L has
// square cells of side c_L = c_0 * 2^L and holds the boxes whose longer side is in (0.875 c_(L-1), 0.875 c_L] (level 0: everything up to
// 0.875 c_0).  c_0 = max(shortest side / 0.875, twice the smaller of the mean spacing sqrt(extent area / boxes) and the geometric mean
// side, 2^-16 of the largest coordinate magnitude, 2^-20 of the longest side): at most 22 levels, and the fp32 rounding of a position stays below 1/16 of any cell.  A level-L
// box that overlaps box i has its centre inside i's extent grown by 0.4375 c_L, so i looks, on every occupied level, at the cells of its
// extent grown by 0.5 c_L: 3 x 3 on its own level, fewer above, more below - work follows the overlapping pairs, whatever the mix of sizes.
// A box with more than 128 cells to visit ("heavy": large next to many small ones) gets a workgroup instead of a thread, and when the cells
// outnumber the higher ranks it scans those instead.
// One table of NB = 2^ceil(log2 M) entries serves all levels: one entry per cell when the occupied levels fit, else (level, cell) is hashed
// (colliding cells only add candidates, which the IoU test rejects).  Membership order inside a cell comes from atomics and does not
// reach the result.
//
// Workspace, all sizes functions of M alone (P2 = keys padded to a power of two):
//   header 512 B | keys u64[P2] | box float4[M] (rank order) | state int[M] | cellid int[M] | items int[M] | heavy int[M]
//   | counts int[NB] | start int[NB + 1] | excl int[M + 1] | block sums int[NB / 2048 + 2]
#include "common.h"
#include "hdyolo.h"

namespace {

typedef unsigned long long u64;

constexpr int SORT_BLOCK = 8192;      // keys one workgroup sorts in LDS (64 KB)
constexpr int SORT_NT = 1024;
constexpr int SCAN_NT = 256, SCAN_PER = 8, SCAN_BLOCK = SCAN_NT * SCAN_PER;
constexpr int HEAVY_BLOCKS = 1024;    // workgroups of a round that walk the list of heavy boxes
constexpr int LIGHT_CELLS = 128;      // a box with more cells than this to visit is heavy
constexpr int HEAVY_BIT = 1 << 30;    // in cellid (table entries < 2^24)
constexpr int HDR_BYTES = 512;
enum { UNDECIDED = 0, KEPT = 1, SUPPRESSED = 2 };
enum { CELL_IMPROPER = -1 };

struct Header {
    unsigned neg_minx, neg_miny, maxx, maxy;      // atomicMax of ordered keys: min(x1), min(y1), max(x2), max(y2) over the proper boxes
    unsigned max_side, neg_min_side;               // longest and shortest "longer side" of a proper box
    unsigned nonfinite;
    unsigned n_proper, n_heavy, level_mask;
    long long log_sum;                             // sum of ilogb(longer side): the geometric mean side, order-independent
    unsigned undecided[3];                         // round r counts into [r % 3], reads [(r + 2) % 3], clears [(r + 1) % 3]
    unsigned last_slot, rounds;
    float c0, inv0, minx, miny;                    // written by params_kernel
    int gx0, gy0, nlevels, direct;                 // direct: written by table_kernel, with level_base
    int level_base[32];                            // direct: first table entry of each occupied level
};
static_assert(sizeof(Header) <= HDR_BYTES, "header");

struct Ws {
    Header* hdr;
    u64* keys;
    float4* box;
    int *state, *cellid, *items, *heavy, *counts, *start, *excl, *bsum;
    int P2, NB;
    size_t bytes;
};


Ws carve(void* base, int M) {
    Ws w;
    int P2 = 1;
    while (P2 < M) P2 <<= 1;
    w.P2 = P2;
    w.NB = P2 < 64 ? 64 : P2;
    const size_t m = (size_t)(M > 0 ? M : 0);
    char* p = (char*)base;
    size_t o = 0;
    w.hdr = (Header*)(p + o); o += HDR_BYTES;
    w.keys = (u64*)(p + o); o += up16((size_t)P2 * 8);
    w.box = (float4*)(p + o); o += m * 16;
    w.state = (int*)(p + o); o += up16(m * 4);
    w.cellid = (int*)(p + o); o += up16(m * 4);
    w.items = (int*)(p + o); o += up16(m * 4);
    w.heavy = (int*)(p + o); o += up16(m * 4);
    w.counts = (int*)(p + o); o += up16((size_t)w.NB * 4);
    w.start = (int*)(p + o); o += up16(((size_t)w.NB + 1) * 4);
    w.excl = (int*)(p + o); o += up16((m + 1) * 4);
    w.bsum = (int*)(p + o); o += up16(((size_t)w.NB / SCAN_BLOCK + 2) * 4);
    w.bytes = o;
    return w;
}

// ascending order-preserving map of the float line to unsigned, and back
__device__ __forceinline__ unsigned ord(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float unord(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

__device__ __forceinline__ unsigned wave_max(unsigned v) {
    for (int m = 32; m > 0; m >>= 1) {
        const unsigned o = (unsigned)__shfl_xor((int)v, m);
        v = o > v ? o : v;
    }
    return v;
}

__device__ __forceinline__ bool finite4(float a, float b, float c, float d) {
    return fabsf(a) <= 3.4028234664e38f && fabsf(b) <= 3.4028234664e38f && fabsf(c) <= 3.4028234664e38f && fabsf(d) <= 3.4028234664e38f;
}

// ---- 1. keys, extent, longest and shortest side, count of proper boxes, non-finite flag.  Grid-stride, one set of atomics per workgroup
// (one per wave on the same few words cost 1.5 ms at 2^20 boxes).
constexpr int KEYS_BLOCKS = 512;
__global__ __launch_bounds__(256) void keys_kernel(const float* __restrict__ rows, int M, int P2, u64* __restrict__ keys, Header* __restrict__ h) {
    __shared__ unsigned red[4][8];
    __shared__ long long red_lg[4];
    unsigned k0 = 0, k1 = 0, k2 = 0, k3 = 0, ks = 0, kn = 0, np = 0, bad = 0;
    long long lg = 0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < P2; i += gridDim.x * 256) {
        u64 key = ~0ull;
        if (i < M) {
            const float* r = rows + (size_t)i * 5;
            const float x1 = r[0], y1 = r[1], x2 = r[2], y2 = r[3];
            key = ((u64)desc_key(r[4]) << 32) | (unsigned)i;
            if (!finite4(x1, y1, x2, y2)) bad = 1;
            else if (x2 > x1 && y2 > y1) {
                const float w = __fsub_rn(x2, x1), hh = __fsub_rn(y2, y1);
                const float side = w > hh ? w : hh;
                if (!(side <= 3.4028234664e38f)) bad = 1;
                else {
                    k0 = max(k0, ord(-x1)); k1 = max(k1, ord(-y1)); k2 = max(k2, ord(x2)); k3 = max(k3, ord(y2));
                    ks = max(ks, ord(side)); kn = max(kn, ord(-side));
                    lg += ilogbf(side);
                    ++np;
                }
            }
        }
        keys[i] = key;
    }
    for (int m = 32; m > 0; m >>= 1) {
        lg += __shfl_xor(lg, m);
        np += (unsigned)__shfl_xor((int)np, m);
        bad |= (unsigned)__shfl_xor((int)bad, m);
    }
    k0 = wave_max(k0); k1 = wave_max(k1); k2 = wave_max(k2); k3 = wave_max(k3); ks = wave_max(ks); kn = wave_max(kn);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[wave][0] = k0; red[wave][1] = k1; red[wave][2] = k2; red[wave][3] = k3; red[wave][4] = ks; red[wave][5] = kn; red[wave][6] = np;
        red[wave][7] = bad;
        red_lg[wave] = lg;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) {
            for (int q = 0; q < 6; ++q) red[0][q] = max(red[0][q], red[w][q]);
            red[0][6] += red[w][6];
            red[0][7] |= red[w][7];
            red_lg[0] += red_lg[w];
        }
        if (red[0][6]) {                                   // proper boxes in this workgroup's share
            atomicMax(&h->neg_minx, red[0][0]); atomicMax(&h->neg_miny, red[0][1]); atomicMax(&h->maxx, red[0][2]); atomicMax(&h->maxy, red[0][3]);
            atomicMax(&h->max_side, red[0][4]); atomicMax(&h->neg_min_side, red[0][5]);
            atomicAdd(&h->n_proper, red[0][6]);
            atomicAdd((unsigned long long*)&h->log_sum, (unsigned long long)red_lg[0]);      // two's complement: a signed sum
        }
        if (red[0][7]) atomicOr(&h->nonfinite, 1u);
    }
}

// ---- 2. bitonic sort, ascending.  Stages whose partner distance fits a workgroup's LDS block run fused (k from k_lo to k_hi, and of each
// k the steps j <= SORT_BLOCK / 2); the others take one launch per (k, j).
__global__ __launch_bounds__(SORT_NT) void sort_local_kernel(u64* __restrict__ keys, int P2, int k_lo, int k_hi) {
    __shared__ u64 l[SORT_BLOCK];
    const int n = P2 < SORT_BLOCK ? P2 : SORT_BLOCK;
    const int base = blockIdx.x * SORT_BLOCK;
    for (int i = threadIdx.x; i < n; i += SORT_NT) l[i] = keys[base + i];
    __syncthreads();
    for (int k = k_lo; k <= k_hi; k <<= 1) {
        for (int j = (k >> 1) < n ? (k >> 1) : (n >> 1); j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < n; i += SORT_NT) {
                const int p = i ^ j;
                if (p > i) {
                    const u64 a = l[i], c = l[p];
                    const bool up = ((base + i) & k) == 0;
                    if ((a > c) == up) { l[i] = c; l[p] = a; }
                }
            }
            __syncthreads();
        }
    }
    for (int i = threadIdx.x; i < n; i += SORT_NT) keys[base + i] = l[i];
}

__global__ __launch_bounds__(256) void sort_global_kernel(u64* __restrict__ keys, int P2, int k, int j) {
    const int t = blockIdx.x * 256 + threadIdx.x;          // one pair per thread
    if (t >= (P2 >> 1)) return;
    const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));    // index with bit j clear
    const int p = i | j;
    const u64 a = keys[i], c = keys[p];
    const bool up = (i & k) == 0;
    if ((a > c) == up) { keys[i] = c; keys[p] = a; }
}

// ---- 3a. the hierarchy of grids (one thread; after keys_kernel)
__global__ void params_kernel(Header* __restrict__ h) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    h->undecided[0] = 0; h->undecided[1] = 0; h->undecided[2] = h->n_proper;
    h->last_slot = 2; h->rounds = 0;
    float c0 = 1.f, minx = 0.f, miny = 0.f;
    int gx = 1, gy = 1, nl = 1;
    if (h->n_proper && !h->nonfinite) {
        minx = -unord(h->neg_minx); miny = -unord(h->neg_miny);
        const float maxx = unord(h->maxx), maxy = unord(h->maxy), smax = unord(h->max_side), smin = -unord(h->neg_min_side);
        const float amax = fmaxf(fmaxf(fabsf(minx), fabsf(maxx)), fmaxf(fabsf(miny), fabsf(maxy)));
        const double area = ((double)maxx - (double)minx) * ((double)maxy - (double)miny);
        const float spacing = (float)fmin(sqrt(area / (double)h->n_proper), 1e38);
        const float typical = fminf(exp2f((float)((double)h->log_sum / (double)h->n_proper) + 0.5f), smax);      // geometric mean of the longer sides
        c0 = fmaxf(fmaxf(smin / 0.875f, 2.f * fminf(spacing, typical)), fmaxf(amax * (1.f / 65536.f), smax * (1.f / 1048576.f)));
        c0 = fminf(fmaxf(c0, 1e-30f), 1e37f);
        const float ex = (maxx * 0.5f - minx * 0.5f) / c0 * 2.f, ey = (maxy * 0.5f - miny * 0.5f) / c0 * 2.f;   // <= 2^17 + rounding
        gx = (int)fminf(fmaxf(floorf(ex), 0.f), 262144.f) + 1;
        gy = (int)fminf(fmaxf(floorf(ey), 0.f), 262144.f) + 1;
        float lim = 0.875f * c0;
        for (nl = 1; smax > lim && nl < 32; ++nl) lim *= 2.f;                 // <= 22 by c0 >= smax * 2^-20
    }
    h->c0 = c0; h->inv0 = 1.f / c0; h->minx = minx; h->miny = miny; h->gx0 = gx; h->gy0 = gy; h->nlevels = nl;
}

struct Grid {
    float c0, inv0, minx, miny;
    int gx0, gy0, direct, mask;
    unsigned levels;
    const int* base;
};
__device__ __forceinline__ Grid load_grid(const Header* h, int NB) {
    Grid g;
    g.c0 = h->c0; g.inv0 = h->inv0; g.minx = h->minx; g.miny = h->miny; g.gx0 = h->gx0; g.gy0 = h->gy0; g.direct = h->direct; g.mask = NB - 1;
    g.levels = h->level_mask; g.base = h->level_base;
    return g;
}
__device__ __forceinline__ int level_of(const Grid& g, float side) {
    float lim = 0.875f * g.c0;
    int L = 0;
    for (; side > lim && L < 31; ++L) lim *= 2.f;
    return L;
}
__device__ __forceinline__ float level_cell(const Grid& g, int L) { return ldexpf(g.c0, L); }
__device__ __forceinline__ int level_gx(const Grid& g, int L) { return ((g.gx0 - 1) >> L) + 1; }
__device__ __forceinline__ int level_gy(const Grid& g, int L) { return ((g.gy0 - 1) >> L) + 1; }
// cell coordinate of a position on level L, clamped into that level's grid (monotone, so neighbours stay neighbours; NaN lands in cell 0)
__device__ __forceinline__ int cell_x(const Grid& g, int L, float x) {
    return (int)fminf(fmaxf(floorf((x - g.minx) * ldexpf(g.inv0, -L)), 0.f), (float)(level_gx(g, L) - 1));
}
__device__ __forceinline__ int cell_y(const Grid& g, int L, float y) {
    return (int)fminf(fmaxf(floorf((y - g.miny) * ldexpf(g.inv0, -L)), 0.f), (float)(level_gy(g, L) - 1));
}
__device__ __forceinline__ int bucket(const Grid& g, int L, int cx, int cy) {
    if (g.direct) return g.base[L] + cy * level_gx(g, L) + cx;               // < sum of the occupied levels' cells <= NB
    return (int)((((unsigned)cx * 73856093u) ^ ((unsigned)cy * 19349663u) ^ ((unsigned)L * 83492791u)) & (unsigned)g.mask);
}
// the cells of level L that box b has to visit: its extent grown by half a cell
struct Range { int x0, y0, nx, ny; };
__device__ __forceinline__ Range visit_range(const Grid& g, int L, const float4& b) {
    const float hc = 0.5f * level_cell(g, L);
    Range r;
    r.x0 = cell_x(g, L, b.x - hc); r.y0 = cell_y(g, L, b.y - hc);
    r.nx = cell_x(g, L, b.z + hc) - r.x0 + 1; r.ny = cell_y(g, L, b.w + hc) - r.y0 + 1;
    return r;
}
__device__ __forceinline__ long long visit_cells(const Grid& g, const float4& b) {
    long long n = 0;
    for (unsigned m = g.levels; m; m &= m - 1) {
        const Range r = visit_range(g, __ffs((int)m) - 1, b);
        n += (long long)r.nx * r.ny;
    }
    return n;
}

// ---- 3b. boxes in rank order, initial state, occupied levels
__global__ __launch_bounds__(256) void gather_kernel(const float* __restrict__ rows, int M, const u64* __restrict__ keys, float4* __restrict__ box,
                                                     int* __restrict__ state, Header* __restrict__ h) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    unsigned bit = 0;
    if (r < M) {
        const float* s = rows + (size_t)(unsigned)(keys[r] & 0xFFFFFFFFull) * 5;
        const float x1 = s[0], y1 = s[1], x2 = s[2], y2 = s[3];
        box[r] = make_float4(x1, y1, x2, y2);
        const bool proper = finite4(x1, y1, x2, y2) && x2 > x1 && y2 > y1;
        state[r] = proper ? UNDECIDED : KEPT;
        if (proper) {
            const float w = __fsub_rn(x2, x1), hh = __fsub_rn(y2, y1);
            float lim = 0.875f * h->c0;
            int L = 0;
            for (const float side = w > hh ? w : hh; side > lim && L < 31; ++L) lim *= 2.f;      // = level_of
            bit = 1u << L;
        }
    }
    for (int m = 32; m > 0; m >>= 1) bit |= (unsigned)__shfl_xor((int)bit, m);
    if ((threadIdx.x & 63) == 0 && (bit & ~h->level_mask)) atomicOr(&h->level_mask, bit);     // (a stale read only costs an atomic)
}

// ---- 3c. one table entry per cell of the occupied levels when they fit, else hashing (one thread; after gather_kernel)
__global__ void table_kernel(Header* __restrict__ h, int NB) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    long long total = 0;
    for (int L = 0; L < 32; ++L) {
        h->level_base[L] = (int)(total < NB ? total : 0);
        if ((h->level_mask >> L) & 1u) total += (long long)(((h->gx0 - 1) >> L) + 1) * (((h->gy0 - 1) >> L) + 1);
    }
    h->direct = total <= (long long)NB ? 1 : 0;
}

// ---- 3d. cell of every box; histogram; list of heavy boxes
__global__ __launch_bounds__(256) void hist_kernel(int M, int NB, const float4* __restrict__ box, const int* __restrict__ state, int* __restrict__ cellid,
                                                   int* __restrict__ counts, int* __restrict__ heavy, Header* __restrict__ h) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    const Grid g = load_grid(h, NB);
    bool is_heavy = false;
    if (r < M) {
        int id = CELL_IMPROPER;
        if (state[r] == UNDECIDED) {
            const float4 b = box[r];
            const float w = __fsub_rn(b.z, b.x), hh = __fsub_rn(b.w, b.y);
            const int L = level_of(g, w > hh ? w : hh);
            id = bucket(g, L, cell_x(g, L, b.x * 0.5f + b.z * 0.5f), cell_y(g, L, b.y * 0.5f + b.w * 0.5f));
            atomicAdd(&counts[id], 1);
            is_heavy = visit_cells(g, b) > LIGHT_CELLS;
            if (is_heavy) id |= HEAVY_BIT;
        }
        cellid[r] = id;
    }
    const u64 m = __ballot(is_heavy);
    if (m) {
        const int lane = threadIdx.x & 63;
        unsigned base = 0;
        if (lane == 0) base = atomicAdd(&h->n_heavy, (unsigned)__popcll(m));
        base = (unsigned)__shfl((int)base, 0);
        if (is_heavy) heavy[base + __popcll(m & ((1ull << lane) - 1ull))] = r;   // n_heavy <= n_proper <= M
    }
}

__global__ __launch_bounds__(256) void scatter_kernel(int M, const int* __restrict__ cellid, const int* __restrict__ start, int* __restrict__ fill,
                                                      int* __restrict__ items) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= M) return;
    const int id = cellid[r];
    if (id < 0) return;
    const int e = id & ~HEAVY_BIT;
    items[start[e] + atomicAdd(&fill[e], 1)] = r;                                // start[e] + count[e] <= start[NB] <= M
}

// ---- exclusive scan of n ints (KEPT_FLAGS: of state[i] == KEPT) into out[0 .. n], out[n] = total.  Three launches: block totals, scan of the
// totals by one workgroup, final pass.
template <bool KEPT_FLAGS>
__device__ __forceinline__ int scan_load(const int* in, int i, int n) {
    if (i >= n) return 0;
    return KEPT_FLAGS ? (in[i] == KEPT ? 1 : 0) : in[i];
}

// exclusive prefix of `v` over the workgroup's threads (SCAN_NT); *total = workgroup sum
__device__ __forceinline__ int block_excl(int v, int* total) {
    __shared__ int wsum[SCAN_NT / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(inc, d);
        if (lane >= d) inc += o;
    }
    __syncthreads();                       // wsum may still be read by a previous call
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int off = 0, tot = 0;
    for (int w = 0; w < SCAN_NT / 64; ++w) {
        if (w < wave) off += wsum[w];
        tot += wsum[w];
    }
    *total = tot;
    return off + inc - v;
}

template <bool KEPT_FLAGS>
__global__ __launch_bounds__(SCAN_NT) void scan_totals_kernel(const int* __restrict__ in, int n, int* __restrict__ bsum) {
    const int i0 = blockIdx.x * SCAN_BLOCK + threadIdx.x * SCAN_PER;
    int s = 0;
    for (int e = 0; e < SCAN_PER; ++e) s += scan_load<KEPT_FLAGS>(in, i0 + e, n);
    int tot;
    block_excl(s, &tot);
    if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

__global__ __launch_bounds__(SCAN_NT) void scan_sums_kernel(int* __restrict__ bsum, int nb) {
    int carry = 0;
    for (int c0 = 0; c0 < nb; c0 += SCAN_NT) {          // uniform trip count
        const int i = c0 + threadIdx.x;
        const int v = i < nb ? bsum[i] : 0;
        int tot;
        const int ex = block_excl(v, &tot);
        if (i < nb) bsum[i] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) bsum[nb] = carry;
}

template <bool KEPT_FLAGS>
__global__ __launch_bounds__(SCAN_NT) void scan_final_kernel(const int* __restrict__ in, int n, const int* __restrict__ bsum, int nb, int* __restrict__ out) {
    const int i0 = blockIdx.x * SCAN_BLOCK + threadIdx.x * SCAN_PER;
    int v[SCAN_PER], s = 0;
    for (int e = 0; e < SCAN_PER; ++e) { v[e] = scan_load<KEPT_FLAGS>(in, i0 + e, n); s += v[e]; }
    int tot;
    int run = bsum[blockIdx.x] + block_excl(s, &tot);
    for (int e = 0; e < SCAN_PER; ++e) {
        if (i0 + e < n) out[i0 + e] = run;
        run += v[e];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) out[n] = bsum[nb];
}

// ---- 4. one round
struct RoundArgs {
    int M, NB, round;
    float iou;
    const float4* box;
    int* state;
    const int *cellid, *items, *start, *heavy;
    Header* h;
};

// candidate j against box i (rank i, b / area): j must rank higher; returns the new knowledge about i
__device__ __forceinline__ void look(const RoundArgs& p, int i, const float4& b, float area, int j, bool& hit_kept, bool& hit_und) {
    if (j >= i) return;
    const int sj = p.state[j];
    if (sj == SUPPRESSED) return;
    const float4 a = p.box[j];
    const float aarea = __fmul_rn(__fsub_rn(a.z, a.x), __fsub_rn(a.w, a.y));
    if (iou_gt(a.x, a.y, a.z, a.w, aarea, b.x, b.y, b.z, b.w, area, p.iou)) {
        if (sj == KEPT) hit_kept = true;
        else hit_und = true;
    }
}

__global__ __launch_bounds__(256) void round_kernel(const RoundArgs p) {
    Header* h = p.h;
    const int cur = p.round % 3, prev = (p.round + 2) % 3, next = (p.round + 1) % 3;
    if (h->undecided[prev] == 0) {                        // written by earlier launches only: the whole grid agrees
        if (blockIdx.x == 0 && threadIdx.x == 0) h->undecided[cur] = 0;      // hand the zero on: the next round reads this slot
        return;
    }
    const int light_blocks = (p.M + 255) / 256;
    if (blockIdx.x == 0 && threadIdx.x == 0) { h->undecided[next] = 0; h->last_slot = (unsigned)cur; h->rounds += 1; }
    const Grid g = load_grid(h, p.NB);

    if ((int)blockIdx.x < light_blocks) {
        // one thread per rank: boxes with few cells to visit
        const int i = blockIdx.x * 256 + threadIdx.x;
        bool waiting = false;
        if (i < p.M && p.state[i] == UNDECIDED && !(p.cellid[i] & HEAVY_BIT)) {      // (undecided boxes are proper: cellid >= 0)
            const float4 b = p.box[i];
            const float area = __fmul_rn(__fsub_rn(b.z, b.x), __fsub_rn(b.w, b.y));
            bool hit_kept = false, hit_und = false;
            for (unsigned m = g.levels; m && !hit_kept; m &= m - 1) {
                const int L = __ffs((int)m) - 1;
                const Range r = visit_range(g, L, b);
                for (int c = 0; c < r.nx * r.ny && !hit_kept; ++c) {                 // <= LIGHT_CELLS
                    const int bk = bucket(g, L, r.x0 + c % r.nx, r.y0 + c / r.nx);
                    const int e = p.start[bk + 1];
                    for (int q = p.start[bk]; q < e && !hit_kept; ++q) look(p, i, b, area, p.items[q], hit_kept, hit_und);
                }
            }
            if (hit_kept) p.state[i] = SUPPRESSED;
            else if (!hit_und) p.state[i] = KEPT;
            else waiting = true;
        }
        const u64 m = __ballot(waiting);
        if (m && (threadIdx.x & 63) == 0) atomicAdd(&h->undecided[cur], (unsigned)__popcll(m));
        return;
    }

    // one workgroup per heavy box
    const int nheavy = (int)h->n_heavy;
    for (int q = blockIdx.x - light_blocks; q < nheavy; q += HEAVY_BLOCKS) {
        const int i = p.heavy[q];
        if (p.state[i] != UNDECIDED) continue;            // written by this workgroup's thread 0 only, in an earlier launch: uniform
        const float4 b = p.box[i];
        const float area = __fmul_rn(__fsub_rn(b.z, b.x), __fsub_rn(b.w, b.y));
        bool hit_kept = false, hit_und = false;
        if (visit_cells(g, b) < (long long)i) {
            for (unsigned m = g.levels; m; m &= m - 1) {
                const int L = __ffs((int)m) - 1;
                const Range r = visit_range(g, L, b);
                const long long n = (long long)r.nx * r.ny;              // < i < 2^24
                for (int c = threadIdx.x; c < (int)n; c += 256) {
                    const int bk = bucket(g, L, r.x0 + c % r.nx, r.y0 + c / r.nx);
                    const int e = p.start[bk + 1];
                    for (int s = p.start[bk]; s < e; ++s) look(p, i, b, area, p.items[s], hit_kept, hit_und);
                }
            }
        } else {
            for (int j = threadIdx.x; j < i; j += 256) look(p, i, b, area, j, hit_kept, hit_und);
        }
        const int any_kept = __syncthreads_or(hit_kept ? 1 : 0);
        const int any_und = __syncthreads_or(hit_und ? 1 : 0);
        if (threadIdx.x == 0) {
            if (any_kept) p.state[i] = SUPPRESSED;
            else if (!any_und) p.state[i] = KEPT;
            else atomicAdd(&h->undecided[cur], 1u);
        }
    }
}

// ---- 5. compaction of the kept flags in rank order
__global__ __launch_bounds__(256) void finish_kernel(int M, int max_det, const int* __restrict__ state, const int* __restrict__ excl,
                                                     const u64* __restrict__ keys, long long* __restrict__ keep, int* __restrict__ n_keep,
                                                     int* __restrict__ status, const Header* __restrict__ h) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int total = excl[M];
    if (i < M && state[i] == KEPT) {
        const int pos = excl[i];
        if (pos < max_det) keep[pos] = (long long)(keys[i] & 0xFFFFFFFFull);
    }
    if (i < max_det && i >= total) keep[i] = -1;
    if (i == 0) {
        n_keep[0] = total < max_det ? total : max_det;
        status[0] = (int)h->undecided[h->last_slot];
        status[1] = (int)h->nonfinite;
        status[2] = (int)h->rounds;
    }
}

template <bool KEPT_FLAGS>
int scan_launch(const int* in, int n, int* bsum, int* out, hipStream_t st, const char* who) {
    const int nb = cdiv(n, SCAN_BLOCK);
    hipLaunchKernelGGL(scan_totals_kernel<KEPT_FLAGS>, dim3(nb), dim3(SCAN_NT), 0, st, in, n, bsum);
    hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(SCAN_NT), 0, st, bsum, nb);
    hipLaunchKernelGGL(scan_final_kernel<KEPT_FLAGS>, dim3(nb), dim3(SCAN_NT), 0, st, in, n, (const int*)bsum, nb, out);
    HDY_LAUNCH_CHECK(who);
    return HDY_OK;
}

}  // namespace

extern "C" {

size_t hdy_nms_grid_workspace_bytes(int M) {
    if (M < 1 || M > HDY_NMS_GRID_MAX_M) return 0;
    return carve(nullptr, M).bytes;
}

int hdy_nms_grid_begin(const float* boxes_scores, int M, void* workspace, size_t ws_bytes, void* stream) {
    HDY_ARG(M >= 1 && M <= HDY_NMS_GRID_MAX_M, "nms_grid_begin: M=%d outside [1, %d]", M, HDY_NMS_GRID_MAX_M);
    HDY_ARG(boxes_scores, "nms_grid_begin: null input");
    HDY_ARG(workspace && ws_bytes >= hdy_nms_grid_workspace_bytes(M), "nms_grid_begin: workspace too small");
    HDY_ARG(((uintptr_t)workspace & 15) == 0, "nms_grid_begin: workspace must be 16-byte aligned");
    const Ws w = carve(workspace, M);
    hipStream_t st = (hipStream_t)stream;
    const char* who = "nms_grid_begin";
    HDY_CHECKED(hdy_memset_async(who, w.hdr, 0, HDR_BYTES, st));
    HDY_CHECKED(hdy_memset_async(who, w.counts, 0, (size_t)w.NB * 4, st));
    hipLaunchKernelGGL(keys_kernel, dim3(min(cdiv(w.P2, 256), KEYS_BLOCKS)), dim3(256), 0, st, boxes_scores, M, w.P2, w.keys, w.hdr);
    hipLaunchKernelGGL(params_kernel, dim3(1), dim3(64), 0, st, w.hdr);
    const int P2 = w.P2, nblk = cdiv(P2, SORT_BLOCK);
    hipLaunchKernelGGL(sort_local_kernel, dim3(nblk), dim3(SORT_NT), 0, st, w.keys, P2, 2, P2 < SORT_BLOCK ? P2 : SORT_BLOCK);
    for (int k = SORT_BLOCK * 2; k <= P2; k <<= 1) {      // P2 <= 2^24
        for (int j = k >> 1; j >= SORT_BLOCK; j >>= 1)
            hipLaunchKernelGGL(sort_global_kernel, dim3(cdiv(P2 >> 1, 256)), dim3(256), 0, st, w.keys, P2, k, j);
        hipLaunchKernelGGL(sort_local_kernel, dim3(nblk), dim3(SORT_NT), 0, st, w.keys, P2, k, k);
    }
    HDY_LAUNCH_CHECK("nms_grid_begin(sort)");
    const int gm = cdiv(M, 256);
    hipLaunchKernelGGL(gather_kernel, dim3(gm), dim3(256), 0, st, boxes_scores, M, (const u64*)w.keys, w.box, w.state, w.hdr);
    hipLaunchKernelGGL(table_kernel, dim3(1), dim3(64), 0, st, w.hdr, w.NB);
    hipLaunchKernelGGL(hist_kernel, dim3(gm), dim3(256), 0, st, M, w.NB, (const float4*)w.box, (const int*)w.state, w.cellid, w.counts, w.heavy, w.hdr);
    HDY_LAUNCH_CHECK(who);
    const int rc = scan_launch<false>(w.counts, w.NB, w.bsum, w.start, st, who);
    if (rc) return rc;
    HDY_CHECKED(hdy_memset_async(who, w.counts, 0, (size_t)w.NB * 4, st));
    hipLaunchKernelGGL(scatter_kernel, dim3(gm), dim3(256), 0, st, M, (const int*)w.cellid, (const int*)w.start, w.counts, w.items);
    HDY_LAUNCH_CHECK(who);
    hdy_note_dispatch("nms_grid");
    return HDY_OK;
}

int hdy_nms_grid_round(int M, float iou, int first_round, int n_rounds, void* workspace, size_t ws_bytes, void* stream) {
    HDY_ARG(M >= 1 && M <= HDY_NMS_GRID_MAX_M, "nms_grid_round: M=%d outside [1, %d]", M, HDY_NMS_GRID_MAX_M);
    HDY_ARG(iou >= 0.f && iou <= 1.f, "nms_grid_round: iou threshold must be in [0,1]");
    HDY_ARG(first_round >= 0 && n_rounds >= 0 && n_rounds <= 65536 && first_round <= (1 << 30), "nms_grid_round: bad round numbers");
    HDY_ARG(workspace && ws_bytes >= hdy_nms_grid_workspace_bytes(M), "nms_grid_round: workspace too small");
    HDY_ARG(((uintptr_t)workspace & 15) == 0, "nms_grid_round: workspace must be 16-byte aligned");
    const Ws w = carve(workspace, M);
    RoundArgs a;
    a.M = M; a.NB = w.NB; a.iou = iou; a.box = w.box; a.state = w.state; a.cellid = w.cellid; a.items = w.items; a.start = w.start; a.heavy = w.heavy;
    a.h = w.hdr;
    for (int r = 0; r < n_rounds; ++r) {
        a.round = first_round + r;
        hipLaunchKernelGGL(round_kernel, dim3(cdiv(M, 256) + HEAVY_BLOCKS), dim3(256), 0, (hipStream_t)stream, a);
    }
    HDY_LAUNCH_CHECK("nms_grid_round");
    return HDY_OK;
}

int hdy_nms_grid_finish(int M, int max_det, long long* keep, int* n_keep, int* status, void* workspace, size_t ws_bytes, void* stream) {
    HDY_ARG(M >= 1 && M <= HDY_NMS_GRID_MAX_M, "nms_grid_finish: M=%d outside [1, %d]", M, HDY_NMS_GRID_MAX_M);
    HDY_ARG(keep && n_keep && status, "nms_grid_finish: null output pointer");
    HDY_ARG(max_det >= 1, "nms_grid_finish: max_det=%d must be positive", max_det);
    HDY_ARG(workspace && ws_bytes >= hdy_nms_grid_workspace_bytes(M), "nms_grid_finish: workspace too small");
    HDY_ARG(((uintptr_t)workspace & 15) == 0, "nms_grid_finish: workspace must be 16-byte aligned");
    const Ws w = carve(workspace, M);
    hipStream_t st = (hipStream_t)stream;
    const int rc = scan_launch<true>(w.state, M, w.bsum, w.excl, st, "nms_grid_finish");
    if (rc) return rc;
    const int n = M > max_det ? M : max_det;
    hipLaunchKernelGGL(finish_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, M, max_det, (const int*)w.state, (const int*)w.excl, (const u64*)w.keys,
                       keep, n_keep, status, (const Header*)w.hdr);
    HDY_LAUNCH_CHECK("nms_grid_finish");
    return HDY_OK;
}

}  // extern "C"
