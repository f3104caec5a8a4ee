// Instance masks scored on the device: the overlap of two label maps as a sparse contingency table (hdy_label_overlap) and the matching behind
// APMeter.add(iou_type='masks') + ap_per_class on it (hdy_mask_ap_match).  Integer work bound by loads, atomics and L2; no MFMA, no LDS-DMA.
//
// The arithmetic is stated in include/hdyolo.h ("mask scoring") and restated in tests/mask_score_ref.py.
//
// overlap_kernel: a wave reads 4 x 64 consecutive entries of BOTH maps (eight 4-byte loads per lane in flight before the first use: the
// memory-level parallelism of two 16-byte loads, with lanes on consecutive entries as the run ballot needs them), maps every label to a row
// of the concatenated arrays or to background, and per 64 entries finds the runs of equal (p, t) with one ballot, as paste.hip's areas_kernel
// does for one map.  The first lane of a run adds the run's length to pred_area[p], to true_area[t] and, when both are rows, to the pair's entry
// of an open-addressing table: the 64-bit key (p << 32 | t) is claimed by atomicCAS with linear probing, the count is an integer atomicAdd.  A
// nucleus of diameter d costs about d runs per side.  Keys only ever go from EMPTY to their final value, so the plain load in front of the CAS can
// at worst see a stale EMPTY, which the CAS corrects.  Integer adds: every count is exact and independent of arrival order; which slot a pair
// lands in is not, so the result is a set.  A full table counts the failed insert in status[1] and writes nothing.
//
// hdy_mask_ap_match: init (one thread per row), two passes with one thread per table slot, then the resolve pass of score.hip (ap_common.h):
//   best pass:   a slot that is a pair (IoU >= pair_iou) with an ignored label sets touched[p]; otherwise an atomicMax of
//                (IoU bits << 32 | ~truth row) on best[p]: the highest IoU, on a tie the lowest truth row (IoU > 0: fp32 bits order as the values);
//   claim pass:  the slot whose key equals best[p] is p's pair: it writes match[p], match_iou[p] and puts p's claim on the truth (atomicMin);
//   resolve:     rules 4 and 5, one thread per prediction.
// A slot's p and t are range-checked before they index anything, so any table content is memory-safe.
//
// Contract: no allocation, everything on the passed stream, no host synchronisation; all argument checks before any launch.
#include "ap_common.h"
#include "hdyolo.h"

namespace {

typedef unsigned long long u64;

constexpr int THREADS = 256;
constexpr int ROWS = 4;                          // 64-entry rows a wave has in flight per step
constexpr u64 EMPTY = ~0ull;                     // no key: p < 2^31, so no pair has it

inline bool pow2(long long v) { return v > 0 && (v & (v - 1)) == 0; }

struct OArgs {
    const int *pm, *tm;
    long long n, seg_elems;
    int n_seg;
    const int *pbase, *tbase;
    int n_pred, n_true;
    int *parea, *tarea;
    u64* keys;
    unsigned* counts;
    unsigned mask;                               // slots - 1
    int* status;                                 // {pairs, overflow}
};

// the 64-bit finalizer of MurmurHash3 (public domain): neighbouring keys (p, t), (p, t + 1) land far apart
__device__ __forceinline__ unsigned slot_hash(u64 k) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return (unsigned)k;
}

__device__ __forceinline__ void pair_add(const OArgs& a, int p, int t, int len) {
    const u64 key = ((u64)(unsigned)p << 32) | (unsigned)t;
    unsigned h = slot_hash(key) & a.mask;
    for (unsigned probe = 0; probe <= a.mask; ++probe, h = (h + 1) & a.mask) {
        u64 cur = __atomic_load_n(&a.keys[h], __ATOMIC_RELAXED);
        if (cur == EMPTY) {
            cur = atomicCAS(&a.keys[h], EMPTY, key);
            if (cur == EMPTY) {
                atomicAdd(&a.status[0], 1);
                cur = key;
            }
        }
        if (cur == key) {
            atomicAdd(&a.counts[h], (unsigned)len);
            return;
        }
    }
    atomicAdd(&a.status[1], 1);
}

// a map entry -> its row of the concatenated array, or -1 (background: negative, or outside [0, rows) after the base)
__device__ __forceinline__ int row_of(int v, const int* __restrict__ base, long long seg, int rows) {
    if (v < 0) return -1;
    const long long r = (long long)v + (base ? base[seg] : 0);
    return r >= 0 && r < rows ? (int)r : -1;
}

__global__ __launch_bounds__(THREADS) void overlap_kernel(const OArgs a) {
    const int lane = threadIdx.x & 63;
    const long long stride = (long long)gridDim.x * THREADS * ROWS;
    for (long long base = ((long long)blockIdx.x * THREADS + (threadIdx.x - lane)) * ROWS; base < a.n; base += stride) {     // wave-uniform
        // the segment of the step's first entry: one 64-bit division per 4 x 64 entries, not one per entry
        long long seg0 = 0, rem0 = 0;
        if (a.n_seg > 0) {
            seg0 = base / a.seg_elems;
            rem0 = base - seg0 * a.seg_elems;
        }
        int pv[ROWS], tv[ROWS];
#pragma unroll
        for (int k = 0; k < ROWS; ++k) {
            const long long i = base + k * 64 + lane;
            pv[k] = i < a.n ? a.pm[i] : -1;
            tv[k] = i < a.n ? a.tm[i] : -1;
        }
#pragma unroll
        for (int k = 0; k < ROWS; ++k) {
            if (base + k * 64 >= a.n) break;                                  // wave-uniform
            // entries at or beyond n are background before their segment is looked at; below n the segment is < n_seg (n = n_seg * seg_elems)
            long long seg = seg0;
            if (a.n_seg > 0) {
                const long long r = rem0 + k * 64 + lane;                     // < seg_elems + 64 * ROWS
                if (a.seg_elems >= 64 * ROWS) seg += r >= a.seg_elems ? 1 : 0;          // a step crosses at most one boundary
                else seg += (unsigned)r / (unsigned)a.seg_elems;              // segments shorter than a step: r < 512, a 32-bit division
            }
            const int p = row_of(pv[k], a.pbase, seg, a.n_pred), t = row_of(tv[k], a.tbase, seg, a.n_true);
            const int pp = __shfl_up(p, 1), tp = __shfl_up(t, 1);
            const bool head = lane == 0 || p != pp || t != tp;
            const u64 heads = __ballot(head);
            if (head && (p >= 0 || t >= 0)) {
                const u64 rest = lane == 63 ? 0ull : heads >> (lane + 1);
                const int len = rest ? __ffsll((unsigned long long)rest) : 64 - lane;
                if (p >= 0) atomicAdd(&a.parea[p], len);
                if (t >= 0) atomicAdd(&a.tarea[t], len);
                if (p >= 0 && t >= 0) pair_add(a, p, t, len);
            }
        }
    }
}

// the rule block, and where the mask form's IoU comes from: the pair table, the areas and rule 2's best word per prediction
struct MArgs : ApRules {
    const u64* keys;
    const unsigned* counts;
    long long slots;
    const int *parea, *tarea;
    int n_pred, n_true;
    u64* best;
};

// slot s as a pair: its rows and IoU; false when the slot is empty, out of range, or below pair_iou (NaN included)
__device__ __forceinline__ bool slot_pair(const MArgs& a, long long s, int& p, int& t, float& iou) {
    const u64 key = a.keys[s];
    if (key == EMPTY) return false;
    const unsigned kp = (unsigned)(key >> 32), kt = (unsigned)key;
    if (kp >= (unsigned)a.n_pred || kt >= (unsigned)a.n_true) return false;
    p = (int)kp;
    t = (int)kt;
    const unsigned inter = a.counts[s];
    const long long uni = (long long)a.parea[p] + (long long)a.tarea[t] - (long long)inter;
    if (inter == 0 || uni <= 0) return false;
    iou = __fdiv_rn(__uint2float_rn(inter), __ll2float_rn(uni));
    return iou >= a.pair_iou;
}

__device__ __forceinline__ u64 best_key(const MArgs& a, int t, float iou) {
    return ((u64)__float_as_uint(iou) << 32) | (0xFFFFFFFFu - (unsigned)a.true_row(t));
}

__global__ __launch_bounds__(THREADS) void init_kernel(const MArgs a) {
    const int i = blockIdx.x * THREADS + threadIdx.x;
    if (i < a.n_pred) {
        a.best[i] = 0;
        a.match[i] = -1;
        a.miou[i] = 0.f;
        a.live[i] = 0;
    }
    if (i < a.n_true) a.claim[i] = EMPTY;
}

__global__ __launch_bounds__(THREADS) void best_kernel(const MArgs a) {
    const long long s = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (s >= a.slots) return;
    int p, t;
    float iou;
    if (!slot_pair(a, s, p, t, iou)) return;
    if (ap_ignored(a, a.pl[p]) || ap_ignored(a, a.tl[t])) a.live[p] = 1;        // touched (every writer stores 1)
    else atomicMax(&a.best[p], best_key(a, t, iou));
}

__global__ __launch_bounds__(THREADS) void claim_kernel(const MArgs a) {
    const long long s = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (s >= a.slots) return;
    int p, t;
    float iou;
    if (!slot_pair(a, s, p, t, iou)) return;
    if (ap_ignored(a, a.pl[p]) || ap_ignored(a, a.tl[t])) return;
    if (a.best[p] != best_key(a, t, iou)) return;
    a.match[p] = t;
    a.miou[p] = iou;
    atomicMin(&a.claim[t], ap_claim_key(a.ps[p], (unsigned)a.pred_row(p)));
}

__global__ __launch_bounds__(THREADS) void resolve_kernel(const MArgs a) {
    const int p = blockIdx.x * THREADS + threadIdx.x;
    if (p < a.n_pred) ap_resolve(a, p);
}

}  // namespace

extern "C" {

size_t hdy_label_overlap_workspace_bytes(long long slots) {
    if (!pow2(slots) || slots > HDY_OVERLAP_MAX_SLOTS) return 0;
    return up16((size_t)slots * 12);             // keys u64[slots] | counts u32[slots]
}

int hdy_label_overlap(const int* pred_map, const int* true_map, long long elems, long long seg_elems, int n_seg, const int* pred_base,
                      const int* true_base, int n_pred, int n_true, int* pred_area, int* true_area, void* table, size_t table_bytes,
                      long long slots, int* status, void* stream) {
    const char* who = "label_overlap";
    HDY_ARG(elems >= 0 && n_pred >= 0 && n_true >= 0 && n_seg >= 0, "%s: negative count (elems=%lld, n_pred=%d, n_true=%d, n_seg=%d)", who, elems,
            n_pred, n_true, n_seg);
    HDY_ARG(elems == 0 || (pred_map && true_map), "%s: null map pointer", who);
    HDY_ARG((pred_area || n_pred == 0) && (true_area || n_true == 0), "%s: null area pointer", who);
    HDY_ARG(status, "%s: null status pointer", who);
    HDY_ARG(n_seg == 0 || (pred_base && true_base), "%s: null segment base pointer with n_seg=%d", who, n_seg);
    HDY_ARG(n_seg == 0 || (seg_elems >= 1 && (unsigned __int128)seg_elems * (unsigned)n_seg == (unsigned __int128)elems),
            "%s: elems=%lld is not n_seg * seg_elems = %d * %lld", who, elems, n_seg, seg_elems);
    HDY_ARG(pow2(slots) && slots <= HDY_OVERLAP_MAX_SLOTS, "%s: slots=%lld is not a power of two in [1, %lld]", who, slots,
            (long long)HDY_OVERLAP_MAX_SLOTS);
    HDY_ARG(table && table_bytes >= hdy_label_overlap_workspace_bytes(slots), "%s: null table or workspace too small (%zu bytes, %lld slots need %zu)",
            who, table_bytes, slots, hdy_label_overlap_workspace_bytes(slots));
    HDY_ARG(((uintptr_t)table & 15) == 0, "%s: the table must be 16-byte aligned", who);
    HDY_ARG((((uintptr_t)pred_map | (uintptr_t)true_map | (uintptr_t)pred_base | (uintptr_t)true_base | (uintptr_t)pred_area | (uintptr_t)true_area |
              (uintptr_t)status) & 3) == 0, "%s: misaligned pointer", who);

    OArgs a;
    a.pm = pred_map; a.tm = true_map; a.n = elems; a.seg_elems = n_seg ? seg_elems : 1; a.n_seg = n_seg;
    a.pbase = n_seg ? pred_base : nullptr; a.tbase = n_seg ? true_base : nullptr;
    a.n_pred = n_pred; a.n_true = n_true; a.parea = pred_area; a.tarea = true_area;
    a.keys = (u64*)table; a.counts = (unsigned*)((char*)table + (size_t)slots * 8); a.mask = (unsigned)(slots - 1); a.status = status;

    hipStream_t st = (hipStream_t)stream;
    HDY_CHECKED(hdy_memset_async(who, a.keys, 0xFF, (size_t)slots * 8, st));
    HDY_CHECKED(hdy_memset_async(who, a.counts, 0, (size_t)slots * 4, st));
    HDY_CHECKED(hdy_memset_async(who, status, 0, 8, st));
    HDY_CHECKED(hdy_memset_async(who, pred_area, 0, (size_t)n_pred * 4, st));
    HDY_CHECKED(hdy_memset_async(who, true_area, 0, (size_t)n_true * 4, st));
    if (elems > 0 && (n_pred > 0 || n_true > 0)) {
        const long long per_block = (long long)THREADS * ROWS;
        const long long blocks = (elems + per_block - 1) / per_block;
        hipLaunchKernelGGL(overlap_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(THREADS), 0, st, a);
    }
    HDY_LAUNCH_CHECK(who);
    hdy_note_dispatch("label_overlap");
    return HDY_OK;
}

size_t hdy_mask_ap_match_workspace_bytes(int n_pred, int n_true) {
    if (n_pred < 0 || n_true < 0) return 0;
    return up16(((size_t)n_pred + (size_t)n_true) * 8 + 16);         // best u64[n_pred] | claim u64[n_true]; never 0 for valid counts
}

int hdy_mask_ap_match(const void* table, size_t table_bytes, long long slots, const int* pred_area, const int* true_area, const float* pred_scores,
                      const long long* pred_labels, const int* pred_row, int n_pred, const long long* true_labels, const int* true_row, int n_true,
                      const float* iouv, int n_iou, float pair_iou, const long long* ignore, int n_ignore, unsigned short* hit, unsigned char* live,
                      int* match, float* match_iou, void* workspace, size_t ws_bytes, void* stream) {
    const char* who = "mask_ap_match";
    HDY_ARG(n_pred >= 0 && n_true >= 0, "%s: negative count (n_pred=%d, n_true=%d)", who, n_pred, n_true);
    HDY_CHECKED(ap_check_rules(who, n_pred, n_true, pred_scores, pred_labels, pred_row, true_labels, true_row, iouv, n_iou, pair_iou, ignore, n_ignore,
                               hit, live, match, match_iou));
    HDY_ARG(pow2(slots) && slots <= HDY_OVERLAP_MAX_SLOTS, "%s: slots=%lld is not a power of two in [1, %lld]", who, slots,
            (long long)HDY_OVERLAP_MAX_SLOTS);
    HDY_ARG(table && table_bytes >= hdy_label_overlap_workspace_bytes(slots), "%s: null table or table too small (%zu bytes, %lld slots need %zu)",
            who, table_bytes, slots, hdy_label_overlap_workspace_bytes(slots));
    HDY_ARG((n_pred == 0 || pred_area) && (n_true == 0 || true_area), "%s: null area pointer", who);
    HDY_ARG(workspace && ws_bytes >= hdy_mask_ap_match_workspace_bytes(n_pred, n_true), "%s: null workspace or workspace too small", who);
    HDY_ARG((((uintptr_t)table | (uintptr_t)workspace) & 15) == 0, "%s: table and workspace must be 16-byte aligned", who);
    HDY_ARG((((uintptr_t)pred_area | (uintptr_t)true_area) & 3) == 0, "%s: misaligned pointer", who);

    MArgs a;
    a.keys = (const u64*)table; a.counts = (const unsigned*)((const char*)table + (size_t)slots * 8); a.slots = slots;
    a.parea = pred_area; a.tarea = true_area; a.n_pred = n_pred; a.n_true = n_true; a.best = (u64*)workspace;
    ap_fill_rules(a, pred_scores, pred_labels, pred_row, true_labels, true_row, iouv, n_iou, pair_iou, ignore, n_ignore, hit, live, match, match_iou,
                  a.best + n_pred);

    hipStream_t st = (hipStream_t)stream;
    const int rows = n_pred > n_true ? n_pred : n_true;
    if (rows > 0) hipLaunchKernelGGL(init_kernel, dim3(cdiv(rows, THREADS)), dim3(THREADS), 0, st, a);
    if (n_pred > 0) {
        if (n_true > 0) {
            const unsigned blocks = (unsigned)((slots + THREADS - 1) / THREADS);
            hipLaunchKernelGGL(best_kernel, dim3(blocks), dim3(THREADS), 0, st, a);
            hipLaunchKernelGGL(claim_kernel, dim3(blocks), dim3(THREADS), 0, st, a);
        }
        hipLaunchKernelGGL(resolve_kernel, dim3(cdiv(n_pred, THREADS)), dim3(THREADS), 0, st, a);
    }
    HDY_LAUNCH_CHECK(who);
    hdy_note_dispatch("mask_ap_match");
    return HDY_OK;
}

}  // extern "C"
