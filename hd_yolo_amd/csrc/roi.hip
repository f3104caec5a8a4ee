// RoIAlign forward / backward on NHWC feature maps and the ReLU backward of the Mask-RCNN head.
//
// roi_align follows the torchvision.ops.roi_align semantics the reference calls with (metayolo/models/yolo_head.py:243,294:
// output (M, M), spatial_scale = 1/stride, sampling_ratio = 2, aligned = ROI_ALIGN = False): per output bin the average of
// sampling_ratio^2 bilinear samples; a sample outside [-1, size] contributes 0, coordinates are clamped to >= 0, and the last
// row/column interpolates with itself.  Output is NHWC [R][P][P][C] so the head's convolutions consume it directly.
// Forward: an HBM-bound gather, one lane per (roi, bin, 8- or 4-channel vector).  The backward accumulates into an fp32 image
// (bf16 has no atomic add and rois overlap), privatised per roi in LDS; hdy_cast_store then writes the plan's gradient buffer.
// tests/test_gpu_roi_direct.py compares every entry point of this file's RoIAlign family with the float64 restatement tests/roi_ref.py.
// Inference over a batch's detections: roi_align_levels_kernel does the same gather for every kept row of the padded NMS result from the level
// that produced it, in compacted order (reference: multiscale_roi_align, yolo_head.py:279-299), and mask_rows_kernel picks each row's mask
// channel behind the head (:346-351).
#include "common.h"
#include "hdyolo.h"

namespace {

template <typename T> struct RT;
template <> struct RT<float> { static constexpr int VE = 4; };
template <> struct RT<bf16_t> { static constexpr int VE = 8; };

template <typename T> __device__ __forceinline__ void ld_vec(const T* p, float* f);
template <> __device__ __forceinline__ void ld_vec<float>(const float* p, float* f) {
    const f32x4 v = *(const f32x4*)p;
#pragma unroll
    for (int i = 0; i < 4; ++i) f[i] = v[i];
}
template <> __device__ __forceinline__ void ld_vec<bf16_t>(const bf16_t* p, float* f) {
    V16 u;
    u.i = *(const i32x4*)p;
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = (float)u.h[i];
}
template <typename T> __device__ __forceinline__ void st_vec(T* p, const float* f);
template <> __device__ __forceinline__ void st_vec<float>(float* p, const float* f) { *(f32x4*)p = f32x4{f[0], f[1], f[2], f[3]}; }
template <> __device__ __forceinline__ void st_vec<bf16_t>(bf16_t* p, const float* f) {
    V16 u;
#pragma unroll
    for (int i = 0; i < 8; ++i) u.h[i] = (bf16_t)f[i];
    *(i32x4*)p = u.i;
}

struct Sample { int y0, x0, y1, x1; float w00, w01, w10, w11; bool ok; };

// torchvision's bilinear_interpolate setup for one sample point
__device__ __forceinline__ Sample sample_at(float y, float x, int H, int W) {
    Sample s;
    s.ok = !(y < -1.0f || y > (float)H || x < -1.0f || x > (float)W);
    if (y <= 0.f) y = 0.f;
    if (x <= 0.f) x = 0.f;
    s.y0 = (int)y;
    s.x0 = (int)x;
    if (s.y0 >= H - 1) { s.y0 = s.y1 = H - 1; y = (float)s.y0; } else s.y1 = s.y0 + 1;
    if (s.x0 >= W - 1) { s.x0 = s.x1 = W - 1; x = (float)s.x0; } else s.x1 = s.x0 + 1;
    const float ly = y - (float)s.y0, lx = x - (float)s.x0, hy = 1.f - ly, hx = 1.f - lx;
    s.w00 = hy * hx; s.w01 = hy * lx; s.w10 = ly * hx; s.w11 = ly * lx;
    return s;
}

struct RoiGeom { int b; float y0, x0, bin_h, bin_w; };

__device__ __forceinline__ RoiGeom roi_geom(const float* roi, float scale, int P, int aligned) {
    RoiGeom g;
    g.b = (int)roi[0];
    const float off = aligned ? 0.5f : 0.0f;
    g.x0 = roi[1] * scale - off;
    g.y0 = roi[2] * scale - off;
    float rw = roi[3] * scale - off - g.x0, rh = roi[4] * scale - off - g.y0;
    if (!aligned) {
        rw = fmaxf(rw, 1.0f);
        rh = fmaxf(rh, 1.0f);
    }
    g.bin_w = rw / (float)P;
    g.bin_h = rh / (float)P;
    return g;
}

// One output bin of one roi for one channel vector: the average of S x S bilinear samples (acc zeroed by the caller; `feat` is the roi's image).
// Shared by the single-level and the multi-level kernel, so both give the same bits for the same roi.
template <typename T>
__device__ __forceinline__ void roi_bin(const T* __restrict__ feat, int ldf, int H, int W, const RoiGeom& g, int ph, int pw, int c0, int S,
                                        float* acc) {
    constexpr int VE = RT<T>::VE;
    for (int iy = 0; iy < S; ++iy) {
        const float y = g.y0 + (float)ph * g.bin_h + ((float)iy + 0.5f) * g.bin_h / (float)S;
        for (int ix = 0; ix < S; ++ix) {
            const float x = g.x0 + (float)pw * g.bin_w + ((float)ix + 0.5f) * g.bin_w / (float)S;
            const Sample s = sample_at(y, x, H, W);
            if (!s.ok) continue;
            float a[VE], b[VE], c[VE], d[VE];
            ld_vec<T>(feat + ((size_t)s.y0 * W + s.x0) * ldf + c0, a);
            ld_vec<T>(feat + ((size_t)s.y0 * W + s.x1) * ldf + c0, b);
            ld_vec<T>(feat + ((size_t)s.y1 * W + s.x0) * ldf + c0, c);
            ld_vec<T>(feat + ((size_t)s.y1 * W + s.x1) * ldf + c0, d);
#pragma unroll
            for (int i = 0; i < VE; ++i) acc[i] += s.w00 * a[i] + s.w01 * b[i] + s.w10 * c[i] + s.w11 * d[i];
        }
    }
    const float inv = 1.0f / (float)(S * S);
#pragma unroll
    for (int i = 0; i < VE; ++i) acc[i] *= inv;
}

template <typename T>
__global__ __launch_bounds__(256) void roi_align_kernel(const T* __restrict__ feat, int ldf, int B, int H, int W, int C, const float* __restrict__ rois,
                                                        int R, float scale, int P, int S, int aligned, T* __restrict__ out) {
    constexpr int VE = RT<T>::VE;
    const int VC = C / VE;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)R * P * P * VC) return;
    const int vc = (int)(idx % VC);
    long long t = idx / VC;
    const int pw = (int)(t % P);
    t /= P;
    const int ph = (int)(t % P);
    const int r = (int)(t / P);
    const RoiGeom g = roi_geom(rois + (size_t)r * 5, scale, P, aligned);
    float acc[VE];
#pragma unroll
    for (int i = 0; i < VE; ++i) acc[i] = 0.f;
    if (g.b >= 0 && g.b < B) roi_bin<T>(feat + (size_t)g.b * H * W * ldf, ldf, H, W, g, ph, pw, vc * VE, S, acc);
    st_vec<T>(out + (((size_t)r * P + ph) * P + pw) * C + vc * VE, acc);
}

// Multi-level form over the padded NMS rows of a batch (Detect.masks_device): one lane per (compacted row, bin, channel vector).  Every
// workgroup rebuilds the prefix of n_keep in LDS (B <= 1024 counts, a scan over 256 partial sums), a lane finds its image by bisection, its
// padded row is b * max_det + (row - prefix[b]), and the row's level picks one of the by-value level records.  Rows at or behind
// min(out_rows, SUM n_keep) are not written; padded rows >= n_keep[b] are never read.  No atomics.
constexpr int LEVELS_MAX = 8;
constexpr int LEVELS_MAX_B = 1024;
struct RoiLevels { hdy_roi_level lv[LEVELS_MAX]; };

template <typename T>
__global__ __launch_bounds__(256) void roi_align_levels_kernel(RoiLevels L, int nl, int C, const float* __restrict__ boxes, const float* __restrict__ level,
                                                               int nex, const int* __restrict__ n_keep, int B, int max_det, int P, int S, int aligned,
                                                               T* __restrict__ out, int out_rows) {
    constexpr int VE = RT<T>::VE;
    __shared__ int pre[LEVELS_MAX_B + 1];            // pre[b] = rows of the images before b
    __shared__ int part[256];
    {
        const int t = threadIdx.x;
        int n4[4], s = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int b = 4 * t + i;
            const int n = b < B ? n_keep[b] : 0;
            n4[i] = n < 0 ? 0 : (n > max_det ? max_det : n);
            s += n4[i];
        }
        part[t] = s;
        __syncthreads();
        const int nt = (B + 3) >> 2;                // threads that hold counts; the partial sums behind them are never used
        for (int off = 1; off < nt; off <<= 1) {    // inclusive scan of the partial sums
            const int v = t >= off ? part[t - off] : 0;
            __syncthreads();
            part[t] += v;
            __syncthreads();
        }
        int run = part[t] - s;
        if (t == 0) pre[0] = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            run += n4[i];
            if (4 * t + i < B) pre[4 * t + i + 1] = run;
        }
        __syncthreads();
    }
    const int total = pre[B];
    const int rows = total < out_rows ? total : out_rows;
    const int VC = C / VE;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)rows * P * P * VC) return;
    const int vc = (int)(idx % VC);
    long long q = idx / VC;
    const int pw = (int)(q % P);
    q /= P;
    const int ph = (int)(q % P);
    const int r = (int)(q / P);
    int lo = 0, hi = B - 1;                          // the image b with pre[b] <= r < pre[b + 1]
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (pre[mid + 1] <= r) lo = mid + 1;
        else hi = mid;
    }
    const size_t src = (size_t)lo * max_det + (r - pre[lo]);
    const float lf = level[src * nex];
    const int l = (lf > -1.0f && lf < (float)nl) ? (int)lf : -1;       // NaN and infinities fail the comparison
    float acc[VE];
#pragma unroll
    for (int i = 0; i < VE; ++i) acc[i] = 0.f;
    if (l >= 0) {
        const T* feat = nullptr;
        int H = 1, W = 1, ldf = 0;
        float scale = 0.f;
#pragma unroll
        for (int k = 0; k < LEVELS_MAX; ++k)         // a select chain: a lane-dependent index into the by-value records would go through scratch
            if (k == l) { feat = (const T*)L.lv[k].feat; H = L.lv[k].H; W = L.lv[k].W; ldf = L.lv[k].ldf; scale = L.lv[k].spatial_scale; }
        const f32x4 bx = *(const f32x4*)(boxes + src * 4);
        const float roi[5] = {(float)lo, bx[0], bx[1], bx[2], bx[3]};
        const RoiGeom g = roi_geom(roi, scale, P, aligned);
        roi_bin<T>(feat + (size_t)lo * H * W * ldf, ldf, H, W, g, ph, pw, vc * VE, S, acc);
    }
    st_vec<T>(out + (((size_t)r * P + ph) * P + pw) * C + vc * VE, acc);
}

// out[r][y][x] = vals[r][y][x][mask_indices[max(labels[r], 0)]], zeros for a negative or out-of-range index (Detect.attach_masks' channel choice)
__global__ __launch_bounds__(256) void mask_rows_kernel(const float* __restrict__ vals, int ldv, int K, const long long* __restrict__ labels,
                                                        const int* __restrict__ mask_indices, int n_idx, long long n, int MM, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long r = i / MM;
    long long lab = labels[r];
    lab = lab < 0 ? 0 : lab;
    const int idx = lab < n_idx ? mask_indices[lab] : -1;
    out[i] = (idx >= 0 && idx < K) ? vals[(size_t)i * ldv + idx] : 0.f;
}

// Backward, privatised per roi and WITHOUT scatter: the bilinear weights of a sample factor into a row weight and a column weight, and
// so does the validity test, hence the gradient of a roi's footprint F (fh x fw feature pixels) is two small matrix products per channel,
//     dF = Wy^T (D Wx),   Wy[ph][fy] = SUM_iy wy(sample row (ph, iy), fy),   Wx[pw][fx] likewise,   D = dout of the roi / S^2  (P x P),
// computed deterministically in LDS by one workgroup per (roi, 32-channel block); only the finished footprint goes to the fp32
// gradient image with one global atomic per pixel and channel (rois overlap).  The matched truths of a nuclei tile are a few feature
// pixels wide, so ~200 bins x 4 samples fall onto a handful of pixels: the first version scattered them with global atomics (8 ms per
// call), the second with LDS atomics into the footprint (1.36 ms per call at B=16, 1280x1280: up to 8 bins in flight hit one address).
// Rois whose footprint exceeds the LDS tile scatter directly (they are large, hence uncontended).  The footprint is the range [min i0, max i1]
// of the roi's valid per-axis samples, found by the workgroup from the very values that fill Wy / Wx; a roi without a valid sample on an
// axis contributes nothing and returns.
constexpr int FT = 24;                   // footprint tile side (feature pixels)
constexpr int CB = 32;                   // channels per workgroup
constexpr int PM = 16;                   // largest output side handled by the footprint path (P = 14 for the mask head)

__device__ __forceinline__ void axis_sample(float v, int size, bool* ok, int* i0, int* i1, float* lo, float* hi) {
    *ok = !(v < -1.0f || v > (float)size);
    if (v <= 0.f) v = 0.f;
    *i0 = (int)v;
    if (*i0 >= size - 1) { *i0 = *i1 = size - 1; v = (float)*i0; } else *i1 = *i0 + 1;
    *hi = v - (float)*i0;                // weight of i1
    *lo = 1.f - *hi;                     // weight of i0
}

// coordinate of sample i of bin pb along one axis: the expression of roi_bin, operation for operation
__device__ __forceinline__ float axis_coord(float o, float bs, int pb, int i, int S) { return o + (float)pb * bs + ((float)i + 0.5f) * bs / (float)S; }

template <typename T>
__global__ __launch_bounds__(256) void roi_align_bwd_tiled_kernel(float* __restrict__ dfeat, int B, int H, int W, int C, const float* __restrict__ rois,
                                                                  float scale, int P, int S, int aligned, const T* __restrict__ dout) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* Wy = sm;                          // [PM][FT]
    float* Wx = Wy + PM * FT;                // [PM][FT]
    float* D = Wx + PM * FT;                 // [P*P][CB]
    float* Tm = D + PM * PM * CB;            // [P][fw][CB]
    const int r = blockIdx.x, c0 = blockIdx.y * CB;
    const int cl = threadIdx.x & (CB - 1), bl = threadIdx.x / CB;      // channel lane, 8 row lanes
    const RoiGeom g = roi_geom(rois + (size_t)r * 5, scale, P, aligned);
    if (g.b < 0 || g.b >= B) return;
    // footprint of the valid samples, rows [fy0, fy1] and columns [fx0, fx1]: the smallest i0 and the largest i1 of the same 2 P S per-axis
    // samples (axis_coord, axis_sample) that fill the weight tables below, so a table write cannot leave [f0, f0 + n).  (A closed form of
    // the top sample, y0 + (P - 0.5 / S) bin, rounds differently from the sample's own expression: once in ~10^6 rois it ends one pixel short.)
    __shared__ int fpt[4];                   // fy0, fy1, fx0, fx1
    if (threadIdx.x < 4) fpt[threadIdx.x] = (threadIdx.x & 1) ? -1 : 0x7fffffff;
    __syncthreads();
    for (int k = threadIdx.x; k < 2 * P * S; k += 256) {
        const bool isx = k >= P * S;
        const int j = isx ? k - P * S : k, pb = j / S;
        bool ok; int i0, i1; float lo, hi;
        axis_sample(axis_coord(isx ? g.x0 : g.y0, isx ? g.bin_w : g.bin_h, pb, j - pb * S, S), isx ? W : H, &ok, &i0, &i1, &lo, &hi);
        if (!ok) continue;
        atomicMin(&fpt[isx ? 2 : 0], i0);
        atomicMax(&fpt[isx ? 3 : 1], i1);
    }
    __syncthreads();
    const int fy0 = fpt[0], fy1 = fpt[1], fx0 = fpt[2], fx1 = fpt[3];
    if (fy1 < fy0 || fx1 < fx0) return;      // an axis without a valid sample: the roi contributes nothing
    const int fh = fy1 - fy0 + 1, fw = fx1 - fx0 + 1;
    const bool tiled = fh <= FT && fw <= FT && P <= PM;
    const float inv = 1.0f / (float)(S * S);
    const bool ch_ok = c0 + cl < C;
    if (!tiled) {
        for (int bin = bl; bin < P * P; bin += 256 / CB) {
            const int ph = bin / P, pw = bin - ph * P;
            const float d = ch_ok ? (float)dout[(((size_t)r * P + ph) * P + pw) * C + c0 + cl] * inv : 0.f;
            for (int iy = 0; iy < S; ++iy) {
                const float y = g.y0 + (float)ph * g.bin_h + ((float)iy + 0.5f) * g.bin_h / (float)S;
                for (int ix = 0; ix < S; ++ix) {
                    const float x = g.x0 + (float)pw * g.bin_w + ((float)ix + 0.5f) * g.bin_w / (float)S;
                    const Sample s = sample_at(y, x, H, W);
                    if (!s.ok || !ch_ok) continue;
                    const size_t base = (size_t)g.b * H * W;
                    atomicAdd(dfeat + (base + (size_t)s.y0 * W + s.x0) * C + c0 + cl, d * s.w00);
                    atomicAdd(dfeat + (base + (size_t)s.y0 * W + s.x1) * C + c0 + cl, d * s.w01);
                    atomicAdd(dfeat + (base + (size_t)s.y1 * W + s.x0) * C + c0 + cl, d * s.w10);
                    atomicAdd(dfeat + (base + (size_t)s.y1 * W + s.x1) * C + c0 + cl, d * s.w11);
                }
            }
        }
        return;
    }
    // axis weight tables: thread t < P builds row t of Wy, thread P <= t < 2P row t - P of Wx (no two threads share an entry)
    if ((int)threadIdx.x < 2 * P) {
        const bool isx = (int)threadIdx.x >= P;
        const int pb = isx ? (int)threadIdx.x - P : (int)threadIdx.x;
        float* row = (isx ? Wx : Wy) + pb * FT;
        const int n = isx ? fw : fh, f0 = isx ? fx0 : fy0, size = isx ? W : H;
        const float o = isx ? g.x0 : g.y0, bs = isx ? g.bin_w : g.bin_h;
        for (int j = 0; j < n; ++j) row[j] = 0.f;
        for (int i = 0; i < S; ++i) {
            const float v = axis_coord(o, bs, pb, i, S);
            bool ok; int i0, i1; float lo, hi;
            axis_sample(v, size, &ok, &i0, &i1, &lo, &hi);
            if (!ok) continue;
            row[i0 - f0] += lo;
            row[i1 - f0] += hi;
        }
    }
    // D: the roi's output gradient, scaled
    for (int bin = bl; bin < P * P; bin += 256 / CB) D[bin * CB + cl] = ch_ok ? (float)dout[((size_t)r * P * P + bin) * C + c0 + cl] * inv : 0.f;
    __syncthreads();
    // Tm[ph][fx][c] = SUM_pw D[ph][pw][c] * Wx[pw][fx]
    for (int o = bl; o < P * fw; o += 256 / CB) {
        const int ph = o / fw, fx = o - ph * fw;
        float acc = 0.f;
        for (int pw = 0; pw < P; ++pw) acc += D[(ph * P + pw) * CB + cl] * Wx[pw * FT + fx];
        Tm[o * CB + cl] = acc;
    }
    __syncthreads();
    // dF[fy][fx][c] = SUM_ph Wy[ph][fy] * Tm[ph][fx][c]  -> one global atomic per footprint pixel and channel
    for (int o = bl; o < fh * fw; o += 256 / CB) {
        const int fy = o / fw, fx = o - fy * fw;
        float acc = 0.f;
        for (int ph = 0; ph < P; ++ph) acc += Wy[ph * FT + fy] * Tm[(ph * fw + fx) * CB + cl];
        if (acc != 0.f && ch_ok) atomicAdd(dfeat + (((size_t)g.b * H + fy0 + fy) * W + fx0 + fx) * C + c0 + cl, acc);
    }
}

// du = y <= 0 ? 0 : dz, a select: a NaN y lets dz through (torch's threshold_backward), a non-finite dz behind y <= 0 gives 0
template <typename T>
__global__ __launch_bounds__(256) void relu_bwd_kernel(const T* __restrict__ dz, const T* __restrict__ y, T* __restrict__ du, long long nvec) {
    constexpr int VE = RT<T>::VE;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += (long long)gridDim.x * blockDim.x) {
        float g[VE], v[VE];
        ld_vec<T>(dz + i * VE, g);
        ld_vec<T>(y + i * VE, v);
#pragma unroll
        for (int k = 0; k < VE; ++k) g[k] = v[k] <= 0.f ? 0.f : g[k];
        st_vec<T>(du + i * VE, g);
    }
}

// dst[m][c] (=|+=) (T)src[m][c]: fp32 accumulation image -> pitched NHWC gradient view
template <typename T>
__global__ __launch_bounds__(256) void cast_store_kernel(const float* __restrict__ src, T* __restrict__ dst, int ldd, long long M, int C, int accumulate) {
    const long long n = M * C;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long m = i / C;
        const int c = (int)(i - m * C);
        T* d = dst + m * ldd + c;
        float v = src[i];
        if (accumulate) v += (float)*d;
        *d = (T)v;
    }
}

}  // namespace

#define ROI_ARGS_OK(C, ldf, VE, ptr) ((C) % (VE) == 0 && (ldf) % (VE) == 0 && (((uintptr_t)(ptr)) & 15) == 0)

extern "C" {

int hdy_roi_align_fwd(const void* feat, int ldf, int B, int H, int W, int C, const float* rois, int R, float spatial_scale, int P,
                      int sampling_ratio, int aligned, void* out, int dtype, void* stream) {
    HDY_ARG(R >= 0 && B > 0 && H > 0 && W > 0 && C > 0 && P > 0 && sampling_ratio > 0, "roi_align_fwd: bad sizes");
    if (R == 0) return HDY_OK;
    const int VE = dtype == HDY_BF16 ? 8 : 4;
    HDY_ARG(feat && rois && out && ROI_ARGS_OK(C, ldf, VE, feat) && (((uintptr_t)out) & 15) == 0, "roi_align_fwd: pointers / channel vectors");
    const long long n = (long long)R * P * P * (C / VE);
    const int grid = (int)((n + 255) / 256);
    if (dtype == HDY_BF16)
        hipLaunchKernelGGL(roi_align_kernel<bf16_t>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)feat, ldf, B, H, W, C, rois, R,
                           spatial_scale, P, sampling_ratio, aligned, (bf16_t*)out);
    else
        hipLaunchKernelGGL(roi_align_kernel<float>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const float*)feat, ldf, B, H, W, C, rois, R,
                           spatial_scale, P, sampling_ratio, aligned, (float*)out);
    hdy_note_dispatch("roi_align");
    HDY_LAUNCH_CHECK("roi_align_fwd");
    return HDY_OK;
}

int hdy_roi_align_levels_fwd(const hdy_roi_level* levels, int nl, int C, const float* boxes, const float* level, int nex, const int* n_keep, int B,
                             int max_det, int P, int sampling_ratio, int aligned, void* out, int out_rows, int dtype, void* stream) {
    HDY_ARG(levels && boxes && level && n_keep && out, "roi_align_levels_fwd: null pointer");
    HDY_ARG(nl >= 1 && nl <= LEVELS_MAX, "roi_align_levels_fwd: %d levels (1 .. %d)", nl, LEVELS_MAX);
    HDY_ARG(B >= 1 && B <= LEVELS_MAX_B, "roi_align_levels_fwd: batch of %d images (1 .. %d)", B, LEVELS_MAX_B);
    HDY_ARG(dtype == HDY_BF16 || dtype == HDY_F32, "roi_align_levels_fwd: dtype %d", dtype);
    const int VE = dtype == HDY_BF16 ? 8 : 4;
    HDY_ARG(C > 0 && C % VE == 0, "roi_align_levels_fwd: C = %d is not a multiple of the %d-channel vector", C, VE);
    HDY_ARG(P >= 1 && max_det >= 1 && out_rows >= 0 && nex >= 1 && sampling_ratio >= 1, "roi_align_levels_fwd: bad sizes (P %d, max_det %d, out_rows %d, nex %d, sampling_ratio %d)",
            P, max_det, out_rows, nex, sampling_ratio);
    HDY_ARG(((((uintptr_t)out) | ((uintptr_t)boxes)) & 15) == 0, "roi_align_levels_fwd: out / boxes are not 16-byte aligned");
    RoiLevels L;
    for (int l = 0; l < LEVELS_MAX; ++l) {
        if (l < nl) {
            L.lv[l] = levels[l];
            HDY_ARG(L.lv[l].feat && L.lv[l].H > 0 && L.lv[l].W > 0 && L.lv[l].ldf >= C && ROI_ARGS_OK(C, L.lv[l].ldf, VE, L.lv[l].feat),
                    "roi_align_levels_fwd: level %d: null / misaligned features, bad size or channel pitch", l);
        } else {
            L.lv[l] = hdy_roi_level{nullptr, 1, 1, 0, 0.f};
        }
    }
    if (out_rows == 0) return HDY_OK;
    const long long n = (long long)out_rows * P * P * (C / VE);
    HDY_ARG((n + 255) / 256 <= 0x7fffffffLL, "roi_align_levels_fwd: %d rows are more than one launch covers", out_rows);
    const int grid = (int)((n + 255) / 256);
    if (dtype == HDY_BF16)
        hipLaunchKernelGGL(roi_align_levels_kernel<bf16_t>, dim3(grid), dim3(256), 0, (hipStream_t)stream, L, nl, C, boxes, level, nex, n_keep, B, max_det,
                           P, sampling_ratio, aligned, (bf16_t*)out, out_rows);
    else
        hipLaunchKernelGGL(roi_align_levels_kernel<float>, dim3(grid), dim3(256), 0, (hipStream_t)stream, L, nl, C, boxes, level, nex, n_keep, B, max_det,
                           P, sampling_ratio, aligned, (float*)out, out_rows);
    hdy_note_dispatch("roi_align_levels");
    HDY_LAUNCH_CHECK("roi_align_levels_fwd");
    return HDY_OK;
}

int hdy_mask_rows(const float* vals, int ldv, int K, const long long* labels, const int* mask_indices, const int* mask_indices_host, int n_idx, int R,
                  int M, float* out, long long out_elems, void* stream) {
    HDY_ARG(vals && labels && mask_indices && out, "mask_rows: null pointer");
    HDY_ARG(K >= 1 && ldv >= K && n_idx >= 1 && R >= 0 && M >= 1, "mask_rows: bad sizes (K %d, ldv %d, n_idx %d, R %d, M %d)", K, ldv, n_idx, R, M);
    HDY_ARG(out_elems == (long long)R * M * M, "mask_rows: out holds %lld elements, the call writes %lld", out_elems, (long long)R * M * M);
    if (mask_indices_host)
        for (int i = 0; i < n_idx; ++i) HDY_ARG(mask_indices_host[i] < K, "mask_rows: mask_indices[%d] = %d with %d mask channels", i, mask_indices_host[i], K);
    if (R == 0) return HDY_OK;
    const long long n = out_elems;
    HDY_ARG((n + 255) / 256 <= 0x7fffffffLL, "mask_rows: %d rows are more than one launch covers", R);
    hipLaunchKernelGGL(mask_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, vals, ldv, K, labels, mask_indices, n_idx, n,
                       M * M, out);
    hdy_note_dispatch("mask_rows");
    HDY_LAUNCH_CHECK("mask_rows");
    return HDY_OK;
}

int hdy_roi_align_bwd(const void* dout, float* dfeat_f32, int B, int H, int W, int C, const float* rois, int R, float spatial_scale, int P,
                      int sampling_ratio, int aligned, int dtype, void* stream) {
    HDY_ARG(R >= 0 && B > 0 && H > 0 && W > 0 && C > 0 && P > 0 && sampling_ratio > 0, "roi_align_bwd: bad sizes");
    if (R == 0) return HDY_OK;
    const int VE = dtype == HDY_BF16 ? 8 : 4;
    HDY_ARG(dout && rois && dfeat_f32 && C % VE == 0 && (((uintptr_t)dout) & 15) == 0, "roi_align_bwd: pointers / channel vectors");
    const dim3 grid(R, (C + CB - 1) / CB);
    const int pp = P <= PM ? P : 1;
    const size_t smem = (size_t)(2 * PM * FT + PM * PM * CB + pp * FT * CB) * sizeof(float);        // Wy, Wx, D, Tm: 70 KB at P = 14
    static PerDeviceOnce attr_once;           // first launch of this instance on any thread
    attr_once.run([&] {
        (void)hipFuncSetAttribute((const void*)roi_align_bwd_tiled_kernel<bf16_t>, hipFuncAttributeMaxDynamicSharedMemorySize, (2 * PM * FT + PM * PM * CB + PM * FT * CB) * 4);
        (void)hipFuncSetAttribute((const void*)roi_align_bwd_tiled_kernel<float>, hipFuncAttributeMaxDynamicSharedMemorySize, (2 * PM * FT + PM * PM * CB + PM * FT * CB) * 4);
    });
    if (dtype == HDY_BF16)
        hipLaunchKernelGGL(roi_align_bwd_tiled_kernel<bf16_t>, grid, dim3(256), smem, (hipStream_t)stream, dfeat_f32, B, H, W, C, rois, spatial_scale, P,
                           sampling_ratio, aligned, (const bf16_t*)dout);
    else
        hipLaunchKernelGGL(roi_align_bwd_tiled_kernel<float>, grid, dim3(256), smem, (hipStream_t)stream, dfeat_f32, B, H, W, C, rois, spatial_scale, P,
                           sampling_ratio, aligned, (const float*)dout);
    hdy_note_dispatch("roi_align_bwd");
    HDY_LAUNCH_CHECK("roi_align_bwd");
    return HDY_OK;
}

int hdy_relu_bwd(const void* dz, const void* y, void* du, long long n, int dtype, void* stream) {
    const int VE = dtype == HDY_BF16 ? 8 : 4;
    HDY_ARG(dz && y && du && n >= 0 && n % VE == 0, "relu_bwd: n must be a multiple of one 16-byte vector");
    if (n == 0) return HDY_OK;
    const long long nvec = n / VE;
    const int grid = (int)((nvec + 255) / 256 > 4096 ? 4096 : (nvec + 255) / 256);
    if (dtype == HDY_BF16)
        hipLaunchKernelGGL(relu_bwd_kernel<bf16_t>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)dz, (const bf16_t*)y, (bf16_t*)du, nvec);
    else
        hipLaunchKernelGGL(relu_bwd_kernel<float>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const float*)dz, (const float*)y, (float*)du, nvec);
    HDY_LAUNCH_CHECK("relu_bwd");
    return HDY_OK;
}

int hdy_cast_store(const float* src, void* dst, int ldd, long long M, int C, int accumulate, int dtype, void* stream) {
    HDY_ARG(src && dst && M >= 0 && C > 0 && ldd >= C, "cast_store: bad args");
    if (M == 0) return HDY_OK;
    const long long n = M * C;
    const int grid = (int)((n + 255) / 256 > 8192 ? 8192 : (n + 255) / 256);
    if (dtype == HDY_BF16)
        hipLaunchKernelGGL(cast_store_kernel<bf16_t>, dim3(grid), dim3(256), 0, (hipStream_t)stream, src, (bf16_t*)dst, ldd, M, C, accumulate);
    else
        hipLaunchKernelGGL(cast_store_kernel<float>, dim3(grid), dim3(256), 0, (hipStream_t)stream, src, (float*)dst, ldd, M, C, accumulate);
    HDY_LAUNCH_CHECK("cast_store");
    return HDY_OK;
}

}  // extern "C"
