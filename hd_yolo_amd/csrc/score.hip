// Detection scoring on the device: the matching behind APMeter (metayolo/models/metrics.py add + ap_per_class) for ragged batches and whole
// slides, without a pair list, a sort or cross-image state (hdy_ap_match).  Scalar integer / fp32 work bound by latency and L2; no MFMA, no LDS-DMA.
//
// Per image, with IoU as utils_general.box_iou computes it on CPU fp32 (every operation rounded on its own):
//   1. a pair (p, t) with IoU < pair_iou (or a NaN IoU) is no pair; a pair whose prediction or truth label is ignored only sets touched[p];
//   2. otherwise p keeps the truth of highest IoU, on a tie the lowest truth row: best[p], best_iou[p];
//   3. truth t is claimed by the prediction of highest score among those with best[p] == t, on a tie the lower prediction row: an
//      order-independent 64-bit atomicMin of (desc_key(score) << 32 | row) on claim[t];
//   4. p is matched iff it won its claim and the labels agree; hit bit j = best_iou[p] >= iouv[j];
//   5. live[p] = !(touched[p] && !matched[p]).
// "row" is the position in the concatenated arrays, or pred_row[p] / true_row[t] when given (a caller that permutes its inputs passes the
// original rows and gets the original results).
//
// Launches: setup (block / chunk prefix sums per image, one workgroup), chunk boxes (bounding box of every truth chunk), match pass (a
// workgroup owns PRED_BLOCK prediction rows of one image, walks that image's truth chunks staged in LDS, best pair in registers, one atomicMin),
// resolve pass (one thread per prediction).  A workgroup skips, without loading it, every truth chunk whose box does not overlap (closed
// intervals) the box of its own prediction block: a pair needs IoU >= pair_iou > 0, hence a positive intersection, hence overlapping extents, so
// skipping cannot change a result.  Boxes with a non-finite coordinate are left out of both boxes and always visited.  On tile-sized images
// this costs nothing; on slide sets in spatially coherent order it removes the O(N * M) term.
//
// Contract: no allocation, everything on the passed stream, no host synchronisation.  Offsets are clamped into [0, capacity] on the device, so
// any offset content is memory-safe; rows outside every image's span (beyond off[B]) are neither read nor written.  Outputs are a pure function
// of the inputs: they do not depend on pruning, chunk size (HDY_AP_CHUNK), launch geometry or atomic arrival order.  match / match_iou / live
// double as the match pass' scratch (best, best_iou, touched) and are rewritten by the resolve pass.
//
// Workspace (hdy_ap_match_workspace_bytes, a function of the three counts alone; MINC = 64, the smallest chunk):
//   header 64 B {chunk pairs visited u64, chunk pairs total u64} | blk_off int[B + 1] | chk_off int[B + 1]
//   | chunk box float4[ceil(true_capacity / MINC) + B] | chunk flag int[same] | claim u64[true_capacity]
#include "ap_common.h"
#include "hdyolo.h"

namespace {

typedef unsigned long long u64;

constexpr int PRED_BLOCK = HDY_AP_PRED_BLOCK;       // prediction rows per workgroup = threads
constexpr int MAX_CHUNK = HDY_AP_TRUE_CHUNK;        // truths staged in LDS at a time (default; HDY_AP_CHUNK: 64, 128 or 256)
constexpr int MIN_CHUNK = 64;
constexpr int HDR_BYTES = 64;
constexpr float INF = __builtin_huge_valf();

struct Header {
    u64 visited, total;
};

struct Ws {
    Header* hdr;
    int *blk_off, *chk_off;
    float4* cbox;
    int* cflag;
    u64* claim;
    int max_blocks, max_chunks;
    size_t bytes;
};

Ws carve(void* base, int B, int pcap, int tcap) {
    Ws w;
    w.max_blocks = cdiv(pcap, PRED_BLOCK) + B;
    w.max_chunks = cdiv(tcap, MIN_CHUNK) + B;
    char* p = (char*)base;
    size_t o = 0;
    w.hdr = (Header*)(p + o); o += HDR_BYTES;
    w.blk_off = (int*)(p + o); o += up16(((size_t)B + 1) * 4);
    w.chk_off = (int*)(p + o); o += up16(((size_t)B + 1) * 4);
    w.cbox = (float4*)(p + o); o += (size_t)w.max_chunks * 16;
    w.cflag = (int*)(p + o); o += up16((size_t)w.max_chunks * 4);
    w.claim = (u64*)(p + o); o += up16((size_t)tcap * 8);
    w.bytes = o;
    return w;
}

// the rule block, and where the box form's IoU comes from: boxes, spans, chunking and the workspace arrays
struct Args : ApRules {
    const float4 *pb, *tb; const int *poff, *toff;
    int pcap, tcap, B, tc, prune, max_blocks, max_chunks;
    Header* hdr; int *blk_off, *chk_off; float4* cbox; int* cflag;
};

// image i's rows [lo, lo + n) of an array of `cap` rows: offsets clamped, so that any content is memory-safe
__device__ __forceinline__ void span(const int* __restrict__ off, int i, int cap, int& lo, int& n) {
    int a = off[i], b = off[i + 1];
    a = a < 0 ? 0 : (a > cap ? cap : a);
    b = b < 0 ? 0 : (b > cap ? cap : b);
    lo = a;
    n = b > a ? b - a : 0;
}

// the image whose range of a non-decreasing prefix array pre[0 .. B] holds v (v < pre[B]): the last i with pre[i] <= v
__device__ __forceinline__ int image_of(const int* __restrict__ pre, int B, int v) {
    int lo = 0, hi = B;                                  // answer in [lo, hi)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (pre[mid] <= v) lo = mid;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ bool finite4(const float4& b) {
    return fabsf(b.x) <= 3.4028234664e38f && fabsf(b.y) <= 3.4028234664e38f && fabsf(b.z) <= 3.4028234664e38f && fabsf(b.w) <= 3.4028234664e38f;
}

// min / max of (x1, y1, x2, y2) and OR of a flag over the wave
__device__ __forceinline__ void wave_box(float& x1, float& y1, float& x2, float& y2, int& flag) {
    for (int m = 32; m > 0; m >>= 1) {
        x1 = fminf(x1, __shfl_xor(x1, m)); y1 = fminf(y1, __shfl_xor(y1, m));
        x2 = fmaxf(x2, __shfl_xor(x2, m)); y2 = fmaxf(y2, __shfl_xor(y2, m));
        flag |= __shfl_xor(flag, m);
    }
}

// ---- 1. per image: workgroups of the match pass and truth chunks, as exclusive prefix sums (clamped to what the launches cover); the header
__global__ __launch_bounds__(256) void setup_kernel(const Args a) {
    __shared__ int wsum[2][4];
    __shared__ u64 tsum[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int carry_b = 0, carry_c = 0;
    u64 total = 0;
    for (int c0 = 0; c0 < a.B; c0 += 256) {                 // uniform trip count
        const int i = c0 + threadIdx.x;
        int nb = 0, nc = 0;
        if (i < a.B) {
            int lo, n;
            span(a.poff, i, a.pcap, lo, n);
            nb = (n + PRED_BLOCK - 1) / PRED_BLOCK;
            span(a.toff, i, a.tcap, lo, n);
            nc = (n + a.tc - 1) / a.tc;
        }
        int ib = nb, ic = nc;
        for (int d = 1; d < 64; d <<= 1) {
            const int ob = __shfl_up(ib, d), oc = __shfl_up(ic, d);
            if (lane >= d) { ib += ob; ic += oc; }
        }
        __syncthreads();
        if (lane == 63) { wsum[0][wave] = ib; wsum[1][wave] = ic; }
        __syncthreads();
        int off_b = 0, off_c = 0, tot_b = 0, tot_c = 0;
        for (int w = 0; w < 4; ++w) {
            if (w < wave) { off_b += wsum[0][w]; off_c += wsum[1][w]; }
            tot_b += wsum[0][w]; tot_c += wsum[1][w];
        }
        if (i < a.B) {
            // (the clamps bind only for offsets that are not a partition of the arrays)
            const int eb = min(carry_b + off_b + ib - nb, a.max_blocks), ec = min(carry_c + off_c + ic - nc, a.max_chunks);
            a.blk_off[i] = eb;
            a.chk_off[i] = ec;
            total += (u64)(min(eb + nb, a.max_blocks) - eb) * (u64)(min(ec + nc, a.max_chunks) - ec);
        }
        carry_b = min(carry_b + tot_b, a.max_blocks);
        carry_c = min(carry_c + tot_c, a.max_chunks);
    }
    for (int m = 32; m > 0; m >>= 1) total += __shfl_xor(total, m);
    if (lane == 0) tsum[wave] = total;
    __syncthreads();
    if (threadIdx.x == 0) {
        a.blk_off[a.B] = carry_b;
        a.chk_off[a.B] = carry_c;
        a.hdr->visited = 0;
        a.hdr->total = tsum[0] + tsum[1] + tsum[2] + tsum[3];
    }
}

// ---- 2. bounding box of every truth chunk over its boxes with finite coordinates; flag = it holds a box with a non-finite one.  One wave per chunk.
__global__ __launch_bounds__(64) void chunk_box_kernel(const Args a) {
    const int c = blockIdx.x;
    if (c >= a.chk_off[a.B]) return;
    const int i = image_of(a.chk_off, a.B, c);
    int lo, n;
    span(a.toff, i, a.tcap, lo, n);
    const int k = c - a.chk_off[i];
    const long long first = (long long)k * a.tc;
    float x1 = INF, y1 = INF, x2 = -INF, y2 = -INF;
    int flag = 0;
    if (first < n) {
        const int j1 = lo + (int)min((long long)n, first + a.tc);
        for (int j = lo + (int)first + (int)threadIdx.x; j < j1; j += 64) {
            const float4 b = a.tb[j];
            if (finite4(b)) { x1 = fminf(x1, b.x); y1 = fminf(y1, b.y); x2 = fmaxf(x2, b.z); y2 = fmaxf(y2, b.w); }
            else flag = 1;
        }
    }
    wave_box(x1, y1, x2, y2, flag);
    if (threadIdx.x == 0) {
        a.cbox[c] = make_float4(x1, y1, x2, y2);
        a.cflag[c] = flag;
    }
}

// the workgroup's image, prediction row and whether the row exists
struct Mine {
    int img, p;
    bool active;
};
__device__ __forceinline__ Mine locate(const Args& a) {
    Mine m;
    m.img = image_of(a.blk_off, a.B, blockIdx.x);
    int lo, n;
    span(a.poff, m.img, a.pcap, lo, n);
    const long long r = (long long)(blockIdx.x - a.blk_off[m.img]) * PRED_BLOCK + threadIdx.x;
    m.active = r < n;
    m.p = m.active ? lo + (int)r : 0;
    return m;
}

// ---- 3. match pass
__global__ __launch_bounds__(PRED_BLOCK) void match_kernel(const Args a) {
    __shared__ float4 l_box[MAX_CHUNK];
    __shared__ float l_area[MAX_CHUNK];
    __shared__ int l_row[MAX_CHUNK];
    __shared__ int l_ign[MAX_CHUNK];
    __shared__ u64 l_mask[PRED_BLOCK / 64];
    __shared__ float l_red[PRED_BLOCK / 64][4];
    __shared__ int l_flag[PRED_BLOCK / 64];
    if ((int)blockIdx.x >= a.blk_off[a.B]) return;
    const Mine me = locate(a);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

    float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
    float area = 0.f;
    bool p_ign = false;
    float x1 = INF, y1 = INF, x2 = -INF, y2 = -INF;
    int bad = 0;
    if (me.active) {
        b = a.pb[me.p];
        area = __fmul_rn(__fsub_rn(b.z, b.x), __fsub_rn(b.w, b.y));
        p_ign = ap_ignored(a, a.pl[me.p]);
        if (finite4(b)) { x1 = b.x; y1 = b.y; x2 = b.z; y2 = b.w; }
        else bad = 1;
    }
    wave_box(x1, y1, x2, y2, bad);
    if (lane == 0) { l_red[wave][0] = x1; l_red[wave][1] = y1; l_red[wave][2] = x2; l_red[wave][3] = y2; l_flag[wave] = bad; }
    __syncthreads();
    for (int w = 0; w < PRED_BLOCK / 64; ++w) {
        x1 = fminf(x1, l_red[w][0]); y1 = fminf(y1, l_red[w][1]); x2 = fmaxf(x2, l_red[w][2]); y2 = fmaxf(y2, l_red[w][3]);
        bad |= l_flag[w];
    }

    int tlo, tn;
    span(a.toff, me.img, a.tcap, tlo, tn);
    const int c_first = a.chk_off[me.img];
    const int nch = min(a.chk_off[me.img + 1] - c_first, (tn + a.tc - 1) / a.tc);
    const bool all = !a.prune || bad;

    float best_iou = 0.f;
    int best = -1, best_row = 0;
    bool touched = false;
    unsigned visited = 0;
    for (int base = 0; base < nch; base += PRED_BLOCK) {          // uniform
        const int c = base + threadIdx.x;
        bool visit = false;
        if (c < nch) {
            visit = all || a.cflag[c_first + c] != 0;
            if (!visit) {
                const float4 cb = a.cbox[c_first + c];
                visit = cb.x <= x2 && x1 <= cb.z && cb.y <= y2 && y1 <= cb.w;
            }
        }
        const u64 m = __ballot(visit);
        __syncthreads();                                          // the masks of the previous group have been read
        if (lane == 0) l_mask[wave] = m;
        __syncthreads();
        for (int w = 0; w < PRED_BLOCK / 64; ++w) {
            for (u64 mask = l_mask[w]; mask; mask &= mask - 1) {  // uniform: the masks are shared
                const int cc = base + w * 64 + (__ffsll((unsigned long long)mask) - 1);
                const int t0 = cc * a.tc;                         // < tn
                const int cnt = min(a.tc, tn - t0);
                ++visited;
                __syncthreads();                                  // the previous chunk has been consumed
                if ((int)threadIdx.x < cnt) {
                    const int g = tlo + t0 + threadIdx.x;
                    const float4 t = a.tb[g];
                    l_box[threadIdx.x] = t;
                    l_area[threadIdx.x] = __fmul_rn(__fsub_rn(t.z, t.x), __fsub_rn(t.w, t.y));
                    l_row[threadIdx.x] = a.true_row(g);
                    l_ign[threadIdx.x] = ap_ignored(a, a.tl[g]) ? 1 : 0;
                }
                __syncthreads();
                if (!me.active) continue;
                for (int q = 0; q < cnt; ++q) {
                    const float4 t = l_box[q];
                    const float xx1 = b.x > t.x ? b.x : t.x, yy1 = b.y > t.y ? b.y : t.y;
                    const float xx2 = b.z < t.z ? b.z : t.z, yy2 = b.w < t.w ? b.w : t.w;
                    const float w_ = __fsub_rn(xx2, xx1), h_ = __fsub_rn(yy2, yy1);
                    if (!(w_ > 0.f && h_ > 0.f)) continue;        // intersection 0 or NaN: IoU is 0, -0 or NaN, never >= pair_iou > 0
                    const float inter = __fmul_rn(w_, h_);
                    const float iou = __fdiv_rn(inter, __fsub_rn(__fadd_rn(area, l_area[q]), inter));
                    if (!(iou >= a.pair_iou)) continue;           // (NaN: no pair)
                    if (p_ign || l_ign[q]) { touched = true; continue; }
                    const int row = l_row[q];
                    if (best < 0 || iou > best_iou || (iou == best_iou && row < best_row)) {
                        best_iou = iou; best = tlo + t0 + q; best_row = row;
                    }
                }
            }
        }
    }
    if (me.active) {
        a.match[me.p] = best;
        a.miou[me.p] = best_iou;
        a.live[me.p] = touched ? 1 : 0;
        if (best >= 0) atomicMin(&a.claim[best], ap_claim_key(a.ps[me.p], (unsigned)a.pred_row(me.p)));
    }
    if (threadIdx.x == 0 && visited) atomicAdd(&a.hdr->visited, (u64)visited);
}

// ---- 4. resolve pass
__global__ __launch_bounds__(PRED_BLOCK) void resolve_kernel(const Args a) {
    if ((int)blockIdx.x >= a.blk_off[a.B]) return;
    const Mine me = locate(a);
    if (me.active) ap_resolve(a, me.p);
}

}  // namespace

extern "C" {

size_t hdy_ap_match_workspace_bytes(int n_img, int pred_capacity, int true_capacity) {
    if (n_img < 0 || pred_capacity < 0 || true_capacity < 0 || n_img > HDY_AP_MAX_ROWS || pred_capacity > HDY_AP_MAX_ROWS || true_capacity > HDY_AP_MAX_ROWS)
        return 0;
    return carve(nullptr, n_img, pred_capacity, true_capacity).bytes;
}

int hdy_ap_match(const float* pred_boxes, const float* pred_scores, const long long* pred_labels, const int* pred_off, const int* pred_row,
                 int pred_capacity, const float* true_boxes, const long long* true_labels, const int* true_off, const int* true_row,
                 int true_capacity, int n_img, const float* iouv, int n_iou, float pair_iou, const long long* ignore, int n_ignore,
                 unsigned short* hit, unsigned char* live, int* match, float* match_iou, void* workspace, size_t ws_bytes, void* stream) {
    const char* who = "ap_match";
    HDY_ARG(n_img >= 0 && pred_capacity >= 0 && true_capacity >= 0, "%s: negative count (n_img=%d, pred_capacity=%d, true_capacity=%d)", who, n_img,
            pred_capacity, true_capacity);
    HDY_ARG(n_img <= HDY_AP_MAX_ROWS && pred_capacity <= HDY_AP_MAX_ROWS && true_capacity <= HDY_AP_MAX_ROWS, "%s: a count exceeds %d", who, HDY_AP_MAX_ROWS);
    HDY_CHECKED(ap_check_rules(who, pred_capacity, true_capacity, pred_scores, pred_labels, pred_row, true_labels, true_row, iouv, n_iou, pair_iou,
                               ignore, n_ignore, hit, live, match, match_iou));
    HDY_ARG(pred_off && true_off, "%s: null offset array", who);
    HDY_ARG((pred_capacity == 0 || pred_boxes) && (true_capacity == 0 || true_boxes), "%s: null box pointer", who);
    HDY_ARG((((uintptr_t)pred_boxes | (uintptr_t)true_boxes) & 15) == 0, "%s: boxes must be 16-byte aligned", who);
    HDY_ARG((((uintptr_t)pred_off | (uintptr_t)true_off) & 3) == 0, "%s: misaligned pointer", who);
    HDY_ARG(workspace && ws_bytes >= hdy_ap_match_workspace_bytes(n_img, pred_capacity, true_capacity), "%s: workspace too small", who);
    HDY_ARG(((uintptr_t)workspace & 15) == 0, "%s: workspace must be 16-byte aligned", who);
    const int tc = hdy_opt(HDY_OPT_AP_CHUNK);
    HDY_ARG(tc == 0 || tc == 64 || tc == 128 || tc == 256, "%s: HDY_AP_CHUNK=%d (0, 64, 128 or 256)", who, tc);

    const Ws w = carve(workspace, n_img, pred_capacity, true_capacity);
    Args a;
    ap_fill_rules(a, pred_scores, pred_labels, pred_row, true_labels, true_row, iouv, n_iou, pair_iou, ignore, n_ignore, hit, live, match, match_iou,
                  w.claim);
    a.pb = (const float4*)pred_boxes; a.poff = pred_off; a.tb = (const float4*)true_boxes; a.toff = true_off;
    a.pcap = pred_capacity; a.tcap = true_capacity; a.B = n_img; a.tc = tc ? tc : MAX_CHUNK; a.prune = hdy_opt(HDY_OPT_AP_NO_PRUNE) ? 0 : 1;
    a.max_blocks = w.max_blocks;                                   // = the match and resolve grids
    a.max_chunks = cdiv(true_capacity, a.tc) + n_img;              // = the chunk-box grid (<= the carved w.max_chunks)
    a.hdr = w.hdr; a.blk_off = w.blk_off; a.chk_off = w.chk_off; a.cbox = w.cbox; a.cflag = w.cflag;

    hipStream_t st = (hipStream_t)stream;
    HDY_CHECKED(hdy_memset_async(who, w.claim, 0xFF, (size_t)true_capacity * 8, st));
    hipLaunchKernelGGL(setup_kernel, dim3(1), dim3(256), 0, st, a);
    if (true_capacity > 0 && n_img > 0) hipLaunchKernelGGL(chunk_box_kernel, dim3(a.max_chunks), dim3(64), 0, st, a);
    if (pred_capacity > 0 && n_img > 0) {
        hipLaunchKernelGGL(match_kernel, dim3(w.max_blocks), dim3(PRED_BLOCK), 0, st, a);
        hipLaunchKernelGGL(resolve_kernel, dim3(w.max_blocks), dim3(PRED_BLOCK), 0, st, a);
    }
    HDY_LAUNCH_CHECK(who);
    hdy_note_dispatch("ap_match");
    return HDY_OK;
}

}  // extern "C"
