// C-ABI entry points of the convolution family that select no kernel (see include/hdyolo.h): options, error text, the dispatch log, the
// small host-side queries (hdy_conv_out_dim, hdy_conv_mtiles, hdy_fastdiv_magic) and weight packing.  The entry points that launch a
// convolution (forward, data gradient, weight gradient) live in conv_dispatch.hip next to their kernel selection.  No allocation, no
// synchronisation; process state = the option table below (atomics, initialised once from the environment), the per-kernel "LDS size attribute set" once-flags, and the thread-local error text / dispatch log.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>

#include "common.h"
#include "hdyolo_internal.h"
#include "hdyolo.h"

int hdy_pack_weight_launch(const hdy_pack_desc& d, hipStream_t st);
int hdy_pack_batch_launch(const hdy_pack_desc* table, int n, int total_blocks, hipStream_t st);

static thread_local char g_err[512] = "";

void hdy_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

namespace {
struct OptDef { const char* name; int def; bool flag; };       // flag: the variable's presence means 1 (its value is not parsed)
const OptDef g_opt_def[HDY_OPT_COUNT] = {
    {"HDY_NO_CLASS_WALK", 0, true}, {"HDY_NO_CONV3X3", 0, true}, {"HDY_C3_GRID", 0, false}, {"HDY_NO_CONV3X3S2", 0, false},
    {"HDY_NO_DGRAD_S2", 0, false}, {"HDY_TILE_INTERLEAVE", 1, false}, {"HDY_NO_BIG_TILES", 0, true}, {"HDY_NO_STEM_KERNEL", 0, true},
    {"HDY_WGRAD_BLOCKS", 512, false}, {"HDY_NO_STEM_WGRAD", 0, true}, {"HDY_NO_WGRAD3X3", 0, true}, 
    {"HDY_LOSS_GRID", 2048, false}, {"HDY_NO_DEEP", 0, true}, {"HDY_NO_WGRAD_DEEP", 0, true}, {"HDY_DEEP_BN", 0, false}, {"HDY_DEEP_DEBUG", 0, false}, {"HDY_DEEP_ALL", 1, false}, {"HDY_DEEP_MIN_TILES", 160, false}, {"HDY_DEEP_WALK", 2, false}, {"HDY_NO_BN_REDUCE4", 0, true},
    {"HDY_WGRAD_TILE", 0, false}, {"HDY_SPPF_NO_KEYS", 0, true}, {"HDY_WGRAD_DEEP_KMIN", 192, false}, {"HDY_NO_CONV3X3_C128", 0, true}, {"HDY_NO_F1X1_96", 0, true},
    {"HDY_AP_CHUNK", 0, false}, {"HDY_AP_NO_PRUNE", 0, true},
};
std::atomic<int> g_opt[HDY_OPT_COUNT];
std::once_flag g_opt_once;
void opt_init() {
    std::call_once(g_opt_once, [] {
        for (int i = 0; i < HDY_OPT_COUNT; ++i) {
            const char* v = getenv(g_opt_def[i].name);
            g_opt[i].store(v ? (g_opt_def[i].flag ? 1 : atoi(v)) : g_opt_def[i].def, std::memory_order_relaxed);
        }
    });
}
int opt_index(const char* name) {
    for (int i = 0; name && i < HDY_OPT_COUNT; ++i)
        if (!strcmp(name, g_opt_def[i].name)) return i;
    return -1;
}
thread_local char g_disp_last[64] = "";
// the log is process-wide (autograd runs the backward launch list on its own thread) and ordered; readers get a thread-local copy
std::mutex g_disp_mu;
char g_disp_log[32768] = "";
size_t g_disp_len = 0;
thread_local char g_disp_copy[32768] = "";
}  // namespace

int hdy_opt(int id) {
    opt_init();
    return g_opt[id].load(std::memory_order_relaxed);
}

void hdy_note_dispatch(const char* what) {
    snprintf(g_disp_last, sizeof(g_disp_last), "%s", what);
    const size_t n = strlen(g_disp_last);
    std::lock_guard<std::mutex> lock(g_disp_mu);
    if (g_disp_len + n + 2 < sizeof(g_disp_log)) {
        memcpy(g_disp_log + g_disp_len, g_disp_last, n);
        g_disp_log[g_disp_len + n] = ';';
        g_disp_log[g_disp_len + n + 1] = 0;
        g_disp_len += n + 1;
    }
}

namespace {

enum { KIND_FWD = 0, KIND_DGRAD = 1, KIND_STEM = 2 };

inline int velems(int dtype) { return dtype == HDY_BF16 ? 8 : 4; }
inline int bke(int dtype) { return 8 * velems(dtype); }
inline size_t esize(int dtype) { return dtype == HDY_BF16 ? 2 : 4; }

// rows (padded to the N-tile) x pitch of one packed block
inline size_t block_elems(int rows, int kd, int dtype) {
    const int bn = hdy_conv_bn_tile(rows);
    return (size_t)round_up(rows, bn) * round_up(kd, bke(dtype));
}

}  // namespace

extern "C" {

const char* hdy_last_error(void) { return g_err; }

// name of the kernel family the last launcher call on this thread picked ("" before the first)
const char* hdy_last_dispatch(void) { return g_disp_last; }

// every pick of every thread since the last hdy_dispatch_log_reset(), in launch order, ';'-separated (first 32 KB)
const char* hdy_dispatch_log(void) {
    std::lock_guard<std::mutex> lock(g_disp_mu);
    memcpy(g_disp_copy, g_disp_log, g_disp_len + 1);
    return g_disp_copy;
}

void hdy_dispatch_log_reset(void) {
    std::lock_guard<std::mutex> lock(g_disp_mu);
    g_disp_log[0] = 0;
    g_disp_len = 0;
    g_disp_last[0] = 0;
}

// process-wide switch by the name of its environment variable (common.h HdyOption); returns the previous value, HDY_EINVAL for an unknown name
int hdy_set_option(const char* name, int value) {
    const int i = opt_index(name);
    HDY_ARG(i >= 0, "set_option: unknown option %s", name ? name : "(null)");
    opt_init();
    return g_opt[i].exchange(value, std::memory_order_relaxed);
}

int hdy_get_option(const char* name) {
    const int i = opt_index(name);
    HDY_ARG(i >= 0, "get_option: unknown option %s", name ? name : "(null)");
    return hdy_opt(i);
}

int hdy_version(void) { return HDY_ABI_VERSION; }

// the reciprocal the conv loader divides by (host-only; exported so that the identity can be tested without a GPU)
int hdy_fastdiv_magic(unsigned d, unsigned* magic, int* shift) {
    HDY_ARG(d > 0 && magic && shift, "fastdiv_magic: d must be positive");
    hdy_magic(d, magic, shift);
    return HDY_OK;
}

int hdy_conv_out_dim(int in, int k, int stride, int pad) { return conv_out_dim(in, k, stride, pad); }

int hdy_conv_mtiles(long long M) { return (int)((M + 127) / 128); }

size_t hdy_conv_pack_elems(int K, int C, int R, int S, int stride, int pad, int kind, int dtype) {
    if (kind == KIND_FWD) return block_elems(K, R * S * C, dtype);
    if (kind == KIND_STEM) return block_elems(K, R * S * 4, dtype);
    if (stride == 1) return block_elems(C, R * S * K, dtype);
    size_t n = 0;
    for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2; ++b) {
            const Axis ah = class_axis(R, pad, a), aw = class_axis(S, pad, b);
            if (ah.taps && aw.taps) n += block_elems(C, ah.taps * aw.taps * K, dtype);
        }
    return n;
}

static hdy_pack_desc make_desc(const float* w_a, int K_a, const float* w_b, int K_b, void* out, int Kl, int C, int R, int S, int transpose,
                               int TH, int TW, int rbase, int rstep, int sbase, int sstep, int stem, int rows_total, int Kdp, int dtype,
                               int first_block) {
    hdy_pack_desc d = {};
    d.w_a = w_a; d.w_b = w_b; d.out = out; d.K_a = K_a; d.K_b = K_b; d.Kl = Kl; d.C = C; d.R = R; d.S = S; d.transpose = transpose;
    d.TH = TH; d.TW = TW; d.rbase = rbase; d.rstep = rstep; d.sbase = sbase; d.sstep = sstep; d.stem = stem; d.rows_total = rows_total;
    d.Kdp = Kdp; d.dtype = dtype; d.first_block = first_block;
    d.nblocks = cdiv((long long)rows_total * Kdp, 2048);      // 256 threads x 8 outputs (conv_wgrad.hip PACK_PER_BLOCK)
    return d;
}

// Logical weight W[K][C][R][S]: rows 0..K_a-1 from w_a, the next K_b rows from w_b (two convs fused along K), remaining rows up to
// K are zero (channel padding, e.g. 39 -> 40 detection outputs).  Describes the packing job(s) for `kind`; returns their number.
int hdy_conv_pack_describe(const float* w_a, int K_a, const float* w_b, int K_b, int K, int C, int R, int S, int stride, int pad, int kind,
                           int dtype, void* out, hdy_pack_desc* descs, int first_block) {
    HDY_ARG(w_a && out && descs && K_a > 0 && K_b >= 0 && K >= K_a + K_b && C > 0 && R > 0 && S > 0, "conv_pack: bad args");
    HDY_ARG((K_b == 0) == (w_b == nullptr), "conv_pack: w_b / K_b mismatch");
    HDY_ARG(stride == 1 || stride == 2, "conv_pack: stride %d unsupported", stride);
    HDY_ARG(dtype == HDY_BF16 || dtype == HDY_F32, "conv_pack: unknown dtype %d", dtype);
    HDY_ARG(((long long)K + 256) * ((long long)R * S * ((long long)C + 256) + 64) < (1LL << 31), "conv_pack: weight too large for 32-bit packing indices");
    if (kind == KIND_FWD || kind == KIND_STEM) {
        const int stem = kind == KIND_STEM;
        HDY_ARG(!stem || (C == 3 && K_b == 0), "conv_pack: stem expects C == 3 and a single weight");
        const int kd = stem ? R * S * 4 : R * S * C;
        const int Kdp = round_up(kd, bke(dtype));
        const int rows_total = round_up(K, hdy_conv_bn_tile(K));
        descs[0] = make_desc(w_a, K_a, w_b, K_b, out, K, C, R, S, 0, R, stem ? 1 : S, 0, 1, 0, 1, stem, rows_total, Kdp, dtype, first_block);
        return 1;
    }
    HDY_ARG(kind == KIND_DGRAD, "conv_pack: unknown kind %d", kind);
    const int rows_total = round_up(C, hdy_conv_bn_tile(C));
    if (stride == 1) {
        const int Kdp = round_up(R * S * K, bke(dtype));
        descs[0] = make_desc(w_a, K_a, w_b, K_b, out, K, C, R, S, 1, R, S, R - 1, -1, S - 1, -1, 0, rows_total, Kdp, dtype, first_block);
        return 1;
    }
    size_t off = 0;
    int n = 0;
    for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2; ++b) {
            const Axis ah = class_axis(R, pad, a), aw = class_axis(S, pad, b);
            if (!ah.taps || !aw.taps) continue;
            const int Kdp = round_up(ah.taps * aw.taps * K, bke(dtype));
            descs[n] = make_desc(w_a, K_a, w_b, K_b, (char*)out + off * esize(dtype), K, C, R, S, 1, ah.taps, aw.taps, ah.rmax, -2, aw.rmax,
                                 -2, 0, rows_total, Kdp, dtype, first_block);
            first_block += descs[n].nblocks;
            off += (size_t)rows_total * Kdp;
            ++n;
        }
    return n;
}

int hdy_conv_pack(const float* w_a, int K_a, const float* w_b, int K_b, int K, int C, int R, int S, int stride, int pad, int kind,
                  int dtype, void* out, void* stream) {
    hdy_pack_desc d[4];
    const int n = hdy_conv_pack_describe(w_a, K_a, w_b, K_b, K, C, R, S, stride, pad, kind, dtype, out, d, 0);
    if (n < 0) return n;
    for (int i = 0; i < n; ++i) {
        const int rc = hdy_pack_weight_launch(d[i], (hipStream_t)stream);
        if (rc) return rc;
    }
    return HDY_OK;
}

int hdy_conv_pack_run(const hdy_pack_desc* descs_device, int ndesc, int total_blocks, void* stream) {
    HDY_ARG(descs_device && ndesc > 0 && total_blocks > 0, "conv_pack_run: bad args");
    return hdy_pack_batch_launch(descs_device, ndesc, total_blocks, (hipStream_t)stream);
}

}  // extern "C"
