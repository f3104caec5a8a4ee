// hd_yolo_amd — shared device/host helpers for the gfx950 (MI355X, CDNA4) kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include <mutex>

#define HDY_OK 0
#define HDY_EINVAL (-1)
#define HDY_EUNSUPPORTED (-2)

enum { HDY_F32 = 0, HDY_BF16 = 1 };

// thread-local error text, returned by hdy_last_error()
void hdy_set_error(const char* fmt, ...);

// Process-wide switches (tests, A/B measurements): kernel selection and launch geometry knobs.  Each has an environment variable that
// sets its initial value (read once, under std::call_once) and can be changed at run time through hdy_set_option(); values are atomics.
// Switches also steer the sizing queries (statistic slabs, workspaces), so change them BEFORE building a plan, never under a live one.
enum HdyOption {
    HDY_OPT_NO_CLASS_WALK,     // HDY_NO_CLASS_WALK: stride-2 dgrad as four launches instead of one class-walking launch
    HDY_OPT_NO_CONV3X3,        // HDY_NO_CONV3X3: filter-resident 3x3 kernel off (generic implicit GEMM instead)
    HDY_OPT_C3_GRID,           // HDY_C3_GRID: workgroups of the filter-resident 3x3 kernel (0 = default)
    HDY_OPT_NO_CONV3X3S2,      // HDY_NO_CONV3X3S2: patch-resident 3x3 / stride-2 forward off (1: both forms, 2: the 64 -> 128 form only)
    HDY_OPT_NO_DGRAD_S2,       // HDY_NO_DGRAD_S2: patch-resident stride-2 data gradient off (1: both forms, 2: the 64 <- 128 form only)
    HDY_OPT_TILE_INTERLEAVE,   // HDY_TILE_INTERLEAVE: tile order of the generic kernel (bit 0: column tiles, bit 1: parity classes)
    HDY_OPT_NO_BIG_TILES,      // HDY_NO_BIG_TILES: never the 256-row tile of the generic kernel
    HDY_OPT_NO_STEM_KERNEL,    // HDY_NO_STEM_KERNEL: patch-resident stem forward off
    HDY_OPT_WGRAD_BLOCKS,      // HDY_WGRAD_BLOCKS: workgroups of the generic weight-gradient kernel (default 512)
    HDY_OPT_NO_STEM_WGRAD,     // HDY_NO_STEM_WGRAD: patch-resident stem weight gradient off
    HDY_OPT_NO_WGRAD3X3,       // HDY_NO_WGRAD3X3: patch-resident 3x3 weight gradient off
    HDY_OPT_LOSS_GRID,         // HDY_LOSS_GRID: workgroups of the detection loss' dense pass (default 2048)
    HDY_OPT_NO_DEEP,           // HDY_NO_DEEP: deep-pipelined 256-row implicit GEMM off (generic kernel instead)
    HDY_OPT_NO_WGRAD_DEEP,     // HDY_NO_WGRAD_DEEP: deep-pipelined 256 x 256 weight gradient off (generic weight gradient instead)
    HDY_OPT_DEEP_BN,           // HDY_DEEP_BN: column tile of the deep-pipelined kernel (0 = by shape, 128, 256)
    HDY_OPT_DEEP_DEBUG,        // HDY_DEEP_DEBUG: timing ablations of the deep-pipelined kernel (bit mask, results wrong; measurement only)
    HDY_OPT_DEEP_ALL,          // HDY_DEEP_ALL: 1 (default) the deep-pipelined kernel takes multi-tap (3x3) layers too, 0 the 1x1 layers only
    HDY_OPT_DEEP_MIN_TILES,    // HDY_DEEP_MIN_TILES: fewest 256-row tiles the deep-pipelined kernel takes a layer with (default 160)
    HDY_OPT_DEEP_WALK,         // HDY_DEEP_WALK: stride-2 data gradients (four-class walk) on the deep pipeline: 0 never, 1 always, 2 (default) with >= 256 output channels
    HDY_OPT_NO_BN_REDUCE4,     // HDY_NO_BN_REDUCE4: BatchNorm-backward statistics pass with 8 channels per lane (the generic form, 120 VGPRs) instead of 4 (72)
    HDY_OPT_WGRAD_TILE,        // HDY_WGRAD_TILE: dW tile of the generic weight-gradient kernel per workgroup: 0 (default) 128 x 128 where K and T*C allow, 64 = 64 x 64 (four times the pixel range per workgroup at the same grid: a quarter of the split slabs, twice the operand fetches)
    HDY_OPT_SPPF_NO_KEYS,      // HDY_SPPF_NO_KEYS: SPPF forward with the float-compare kernels instead of the order-preserving 16-bit keys (A/B)
    HDY_OPT_WGRAD_DEEP_KMIN,   // HDY_WGRAD_DEEP_KMIN: fewest output channels (a multiple of 64) the deep-pipelined multi-tap weight gradient takes (default 192; 256 = rounds 3-5)
    HDY_OPT_NO_CONV3X3_C128,   // HDY_NO_CONV3X3_C128: filter-resident 3x3 kernel for 128 input channels off (deep-pipelined / generic kernel instead)
    HDY_OPT_NO_F1X1_96,        // HDY_NO_F1X1_96: fused 1x1 backward instance for 96 channels off (three launches instead; A/B)
    HDY_OPT_AP_CHUNK,          // HDY_AP_CHUNK: truths the AP match pass stages in LDS at a time (0 = default 256; 64, 128, 256): results do not depend on it
    HDY_OPT_AP_NO_PRUNE,       // HDY_AP_NO_PRUNE: the AP match pass visits every truth chunk (A/B, tests: results do not depend on it)
    HDY_OPT_COUNT
};
int hdy_opt(int id);

// thread-local dispatch log: every host-side launcher names the kernel family it picked (hdy_last_dispatch / hdy_dispatch_log)
void hdy_note_dispatch(const char* what);

#define HDY_ARG(cond, ...)                 \
    do {                                   \
        if (!(cond)) {                     \
            hdy_set_error(__VA_ARGS__);    \
            return HDY_EINVAL;             \
        }                                  \
    } while (0)

// return a failed check's status from the entry point (the check has set the error text)
#define HDY_CHECKED(call) do { const int rc__ = (call); if (rc__ != HDY_OK) return rc__; } while (0)

#define HDY_LAUNCH_CHECK(what)                                                      \
    do {                                                                             \
        hipError_t e__ = hipGetLastError();                                          \
        if (e__ != hipSuccess) {                                                     \
            hdy_set_error("%s: launch failed: %s", what, hipGetErrorString(e__));    \
            return (int)e__;                                                         \
        }                                                                            \
    } while (0)

typedef __bf16 bf16_t;
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

// One-time per-kernel setup that is bound to a DEVICE (hipFuncSetAttribute: dynamic LDS above 64 KB): once per process and device, not once per
// process — a second device in the same process (one plan per device; the executor keeps per-device events for that case) would otherwise launch
// without the attribute.
// Sum over the 16 lanes of a DPP row (lanes 16k .. 16k + 15), delivered to every lane of the row: four v_add_f32 with row_ror operands, no LDS
// crossbar.  The BatchNorm sums of the conv epilogues end in this reduction (pixel lanes of an MFMA accumulator tile); as `u += __shfl_xor(u, m)`
// hipcc emitted ds_bpermute_b32 + s_waitcnt lgkmcnt(0) per step and value, one after the other: 64 LDS round trips = 3.2 us for the 32 sums at the
// end of every conv_deep forward launch (profiles/r05_small_probes_ab.txt).
#if defined(__HIPCC__)
__device__ __forceinline__ float row_sum16(float v) {
#ifdef HDY_ROW_SUM_SHFL      // A/B build: the former shuffle chain
    for (int m = 1; m < 16; m <<= 1) v += __shfl_xor(v, m);
    return v;
#endif
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x128, 0xF, 0xF, true));   // row_ror:8
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x124, 0xF, 0xF, true));   // row_ror:4
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x122, 0xF, 0xF, true));   // row_ror:2
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x121, 0xF, 0xF, true));   // row_ror:1
    return v;
}
#endif

struct PerDeviceOnce {
    std::once_flag flag[16];
    template <typename F> void run(F&& fn) {
        int dev = 0;
        (void)hipGetDevice(&dev);
        std::call_once(flag[dev & 15], fn);
    }
};

static inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }
static inline int round_up(int a, int b) { return (a + b - 1) / b * b; }
static inline size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

// hipMemsetAsync of `bytes` (none: no call) on the stream; a failure sets the error text and is returned as the HIP status (HDY_CHECKED)
static inline int hdy_memset_async(const char* who, void* p, int v, size_t bytes, hipStream_t st) {
    if (bytes == 0) return HDY_OK;
    const hipError_t e = hipMemsetAsync(p, v, bytes, st);
    if (e != hipSuccess) {
        hdy_set_error("%s: hipMemsetAsync failed: %s", who, hipGetErrorString(e));
        return (int)e;
    }
    return HDY_OK;
}

#ifdef __HIPCC__
// 16-byte vector <-> 8 bf16 / 4 f32 views
union V16 {
    i32x4 i;
    f32x4 f;
    bf16x8 h;
};

__device__ __forceinline__ float silu_f(float u) { return u / (1.0f + __expf(-u)); }
__device__ __forceinline__ float sigmoid_f(float u) { return 1.0f / (1.0f + __expf(-u)); }

template <typename T> __device__ __forceinline__ float to_f32(T v);
template <> __device__ __forceinline__ float to_f32<float>(float v) { return v; }
template <> __device__ __forceinline__ float to_f32<bf16_t>(bf16_t v) { return (float)v; }
template <typename T> __device__ __forceinline__ T from_f32(float v);
template <> __device__ __forceinline__ float from_f32<float>(float v) { return v; }
template <> __device__ __forceinline__ bf16_t from_f32<bf16_t>(float v) { return (bf16_t)v; }

// Bijective XCD-aware remap of a 1-D grid (cdna_hip_programming.md §5.5 T1): blocks that the
// dispatcher deals to one XCD (same id % 8) get a contiguous range of logical tile ids, so
// neighbouring tiles share that XCD's L2.  Speed only; any mapping is correct.
__device__ __forceinline__ int xcd_remap(int id, int n) {
    const int q = n >> 3, r = n & 7, x = id & 7, s = id >> 3;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + s;
}
// ---- device helpers shared by several kernel files ------------------------------------------------------------------------------------------
// n / d for n < 2^31 with the host-made reciprocal of hdy_magic(): mulhi(2n, mg) >> sh
__device__ __forceinline__ unsigned fdiv(unsigned n, unsigned mg, int sh) { return __umulhi(n << 1, mg) >> sh; }

// ---- NMS arithmetic shared by detect.hip (one workgroup per box set) and nms_grid.hip (one set over the whole chip): the two must agree bit
// for bit, so there is one copy.
// IoU(a, b) > thr in IEEE fp32 with explicit round-to-nearest ops (no FMA contraction), the oracle's operation order; area = (x2 - x1) * (y2 - y1).
__device__ __forceinline__ bool iou_gt(float ax1, float ay1, float ax2, float ay2, float aarea, float bx1, float by1, float bx2, float by2,
                                       float barea, float thr) {
    const float xx1 = ax1 > bx1 ? ax1 : bx1;
    const float yy1 = ay1 > by1 ? ay1 : by1;
    const float xx2 = ax2 < bx2 ? ax2 : bx2;
    const float yy2 = ay2 < by2 ? ay2 : by2;
    float w = __fsub_rn(xx2, xx1);
    float h = __fsub_rn(yy2, yy1);
    w = w < 0.f ? 0.f : w;
    h = h < 0.f ? 0.f : h;
    const float inter = __fmul_rn(w, h);
    const float ovr = __fdiv_rn(inter, __fsub_rn(__fadd_rn(aarea, barea), inter));
    return ovr > thr;
}

// 32-bit key whose ASCENDING unsigned order is DESCENDING score order for every float (negative scores included: explicit-box calls
// carry caller scores of any sign; -0.0 ranks as +0.0).  For the positive scores of the thresholded paths this is ~bits, as before.
__device__ __forceinline__ unsigned desc_key(float s) {
    unsigned u = s == 0.0f ? 0u : __float_as_uint(s);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);      // ascending order-preserving map of the float line
    return ~u;
}

// LDS-DMA straight from global memory: lane l's 16 bytes at g land at lds_wave_base + l*16
__device__ __forceinline__ void glds16(const void* g, unsigned char* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1)))*)g,
                                     (void __attribute__((address_space(3)))*)lds_wave_base, 16, 0, 0);
}

// LDS-DMA through a buffer descriptor: lane l's 16 bytes at base + voff + soff land at lds + l*16; a lane whose offset fails the
// descriptor's range check (>= num_records) gets zeros.
__device__ __forceinline__ void lds_dma16(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff, unsigned char* lds_wave_base) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (void __attribute__((address_space(3)))*)lds_wave_base, 16, (int)voff, (int)soff, 0, 0);
}

// ... with the LDS destination as a byte address
__device__ __forceinline__ void lds_dma16(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff, unsigned lds_byte) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (void __attribute__((address_space(3)))*)(uintptr_t)lds_byte, 16, (int)voff, (int)soff, 0, 0);
}

// 32-byte-block (fsw) and 16-byte-chunk (fsw3) XOR swizzles of the [rows][128 B] LDS sub-tiles of the weight-gradient / fused 1x1 backward kernels
__device__ __forceinline__ int fsw(int row) { return ((row >> 1) & 1) | (((row >> 3) & 1) << 1); }
__device__ __forceinline__ int fsw3(int row) { return (row & 6) ^ (((row >> 3) & 1) * 5); }

// v_exp_f32 + v_rcp_f32 (1 ulp): plenty for activations and far cheaper than the IEEE division sequence
__device__ __forceinline__ float fast_sigmoid(float u) { return __builtin_amdgcn_rcpf(1.0f + __expf(-u)); }
__device__ __forceinline__ float dsilu_f(float u) {
    const float s = fast_sigmoid(u);
    return s * (1.0f + u * (1.0f - s));
}

// 16 bytes of T <-> fp32 values; VEC_OK: rows of `ld` elements at `ptr` can be moved in such vectors
template <typename T> __device__ __forceinline__ void unpack(const i32x4& v, float* f);
template <> __device__ __forceinline__ void unpack<float>(const i32x4& v, float* f) {
    V16 u; u.i = v;
#pragma unroll
    for (int i = 0; i < 4; ++i) f[i] = u.f[i];
}
template <> __device__ __forceinline__ void unpack<bf16_t>(const i32x4& v, float* f) {
    V16 u; u.i = v;
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = (float)u.h[i];
}
template <typename T> __device__ __forceinline__ i32x4 pack(const float* f);
template <> __device__ __forceinline__ i32x4 pack<float>(const float* f) {
    V16 u;
#pragma unroll
    for (int i = 0; i < 4; ++i) u.f[i] = f[i];
    return u.i;
}
template <> __device__ __forceinline__ i32x4 pack<bf16_t>(const float* f) {
    V16 u;
#pragma unroll
    for (int i = 0; i < 8; ++i) u.h[i] = (bf16_t)f[i];
    return u.i;
}

#define VEC_OK(ptr, ld, VE) ((((uintptr_t)(ptr)) & 15) == 0 && (ld) % (VE) == 0)

// LDS fragment reads and barriers of the patch-resident stride-2 kernels (conv3x3s2.hip, conv_dgrad_s2.hip; `HAND`, `smem`, `lds0` are the
// kernel's): as inline asm with hand-counted waits where HAND, else compiler-visible
#define S2_LDSR(dst, addr)                                                                             \
    do {                                                                                               \
        if constexpr (HAND) asm volatile("ds_read_b128 %0, %1" : "=v"(dst) : "v"(addr) : "memory");    \
        else dst = *(const i32x4*)(smem + ((addr) - lds0));                                            \
    } while (0)
#define S2_LGKM(n)                                                                                                       \
    do {                                                                                                                 \
        if constexpr (HAND) { asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(n) : "memory"); __builtin_amdgcn_sched_barrier(0); } \
    } while (0)
#define S2_BARRIER(lg)                                                                                                   \
    do {                                                                                                                 \
        if constexpr (HAND) { if (lg) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_s_barrier(); asm volatile("" ::: "memory"); } \
        else __syncthreads();                                                                                            \
    } while (0)
#endif
