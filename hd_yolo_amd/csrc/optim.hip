// SGD | Adam | AdamW over MANY parameter tensors, plus the weight EMA, in ONE launch: hdy_opt_step (reference: train.py:208-233 builds one of
// the three optimizers over three parameter groups and steps it at train.py:478; :249 / :480 ModelEMA.update after every step,
// common.py:128-155; torch's multi-tensor SGD alone is ~25 launches of 5-25 us for yolov5s' 180 tensors).
//
// The table.  One device row per tensor (hdy_opt_desc: parameter, gradient, two states, EMA destination, length, slot, first, first block),
// built once and replayed while no pointer moves.  A block owns 4096 consecutive elements of one tensor and finds its row by binary search over
// the first-block column.  g == NULL makes an EMA-only row (BatchNorm running statistics, frozen or gradient-less parameters).  The
// hyper-parameters travel by value, one slot per (parameter group, step count): the warm-up rewrites them every step and the table stays.
// The algorithm and "the table has EMA destinations" are template parameters: uniform over the launch, otherwise tested per element.
//
// The arithmetic.  SGD as torch.optim.SGD, in plain expressions compiled with -ffp-contract=off:
//   g' = g + wd*p;   buf = first ? g' : momentum*buf + (1 - dampening)*g';   p -= lr * (nesterov ? g' + momentum*buf : buf)
// Adam as torch.optim.adam's single-tensor path, with explicit fused multiply-adds and correctly rounded division / square root, so the
// result does not depend on compiler flags:
//   AdamW: p *= 1 - lr*wd;  Adam: g += wd*p;  m += (g - m)*(1 - beta1);  v = beta2*v + (1 - beta2)*g*g;
//   p -= (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps)
// and the EMA of what was just written: ema = d*ema + (1 - d)*p.
//
// Pure HBM streaming: p, g, m (, v, ema) are each read once and p, m (, v, ema) written once.  SGD 20 B per parameter, 28 B with the EMA;
// Adam 28 B, 36 B with the EMA; 12 B per EMA-only entry.
#include "common.h"
#include "hdyolo.h"

namespace {

constexpr int OPT_BLOCK_ELEMS = 4096;

// one element of SGD (damp = 1 - dampening; has_buf: the row has a momentum buffer)
__device__ __forceinline__ void sgd_update(float pv, float gv, float bv, float& po, float& bo, float lr, float mom, float damp, float wd, bool has_buf,
                                           int first, int nesterov) {
    if (wd != 0.0f) gv = gv + wd * pv;
    if (has_buf) {
        bo = first ? gv : mom * bv + damp * gv;
        gv = nesterov ? gv + mom * bo : bo;
    }
    po = pv - lr * gv;
}

struct OptHyper {
    float v[HDY_OPT_MAX_SLOTS][HDY_OPT_HYPER];
    float ema_d, ema_omd;
    int nesterov;
};

template <int ALGO, bool EMA>
__global__ __launch_bounds__(256) void opt_step_kernel(const hdy_opt_desc* __restrict__ table, int ndesc, OptHyper h) {
    int lo = 0, hi = ndesc - 1;                           // last descriptor whose first_block <= blockIdx.x
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].first_block <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const hdy_opt_desc d = table[lo];
    const long long base = (long long)((int)blockIdx.x - d.first_block) * OPT_BLOCK_ELEMS;
    const float* hv = h.v[d.slot];
    const float h0 = hv[0], h1 = hv[1], h2 = hv[2], h3 = hv[3], h4 = hv[4], h5 = hv[5], h6 = hv[6];
    float* __restrict__ p = d.p;
    const float* __restrict__ g = d.g;
    float* __restrict__ m = d.m;
    float* __restrict__ v = ALGO == HDY_OPT_SGD ? nullptr : d.v;
    float* __restrict__ e = EMA ? d.ema : nullptr;
    if (!g && !e) return;                                 // nothing to write (the binding refuses such a row)
    const bool ldm = m && !d.first, ldv = v && !d.first;
    // one element: pv / mv / vv in, the new values out (mo / vo only where the row has that state)
    auto upd = [&](float pv, float gv, float mv, float vv, float& po, float& mo, float& vo) {
        if constexpr (ALGO == HDY_OPT_SGD) {
            sgd_update(pv, gv, mv, po, mo, h0, h2, 1.0f - h3, h1, m != nullptr, d.first, h.nesterov);      // slot = {lr, weight_decay, momentum, dampening}
        } else {                                          // slot = {lr / bc1, AdamW: 1 - lr*wd | Adam: wd, 1 - beta1, beta2, 1 - beta2, sqrt(bc2), eps}
            if constexpr (ALGO == HDY_OPT_ADAMW) pv = __fmul_rn(pv, h1);
            else if (h1 != 0.0f) gv = __fmaf_rn(h1, pv, gv);
            mo = __fmaf_rn(__fsub_rn(gv, mv), h2, mv);
            vo = __fmaf_rn(h4, __fmul_rn(gv, gv), __fmul_rn(h3, vv));
            const float denom = __fadd_rn(__fdiv_rn(__fsqrt_rn(vo), h5), h6);
            po = __fmaf_rn(-h0, __fdiv_rn(mo, denom), pv);
        }
    };
    auto ema = [&](float ev, float pn) { return __fmaf_rn(h.ema_d, ev, __fmul_rn(h.ema_omd, pn)); };
    const uintptr_t ptrs = ((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v) | ((uintptr_t)e);
    const bool vec = (d.n & 3) == 0 && (ptrs & 15) == 0;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    if (vec) {
#pragma unroll
        for (int r = 0; r < OPT_BLOCK_ELEMS / 1024; ++r) {
            const long long i = base + (long long)(r * 256 + (int)threadIdx.x) * 4;
            if (i >= d.n) break;
            f32x4 po = *(const f32x4*)(p + i);
            if (g) {
                const f32x4 pv = po, gv = *(const f32x4*)(g + i);
                const f32x4 mv = ldm ? *(const f32x4*)(m + i) : zero, vv = ldv ? *(const f32x4*)(v + i) : zero;
                f32x4 mo = mv, vo = vv;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float pe, me = mv[k], ve = vv[k];
                    upd(pv[k], gv[k], mv[k], vv[k], pe, me, ve);
                    po[k] = pe;
                    mo[k] = me;
                    vo[k] = ve;
                }
                *(f32x4*)(p + i) = po;
                if (m) *(f32x4*)(m + i) = mo;
                if (v) *(f32x4*)(v + i) = vo;
            }
            if (e) {
                f32x4 ev = *(const f32x4*)(e + i);
#pragma unroll
                for (int k = 0; k < 4; ++k) ev[k] = ema(ev[k], po[k]);
                *(f32x4*)(e + i) = ev;
            }
        }
    } else {
        for (int r = 0; r < OPT_BLOCK_ELEMS / 256; ++r) {
            const long long i = base + r * 256 + (int)threadIdx.x;
            if (i >= d.n) break;
            float po = p[i];
            if (g) {
                float mo = 0.f, vo = 0.f;
                upd(po, g[i], ldm ? m[i] : 0.f, ldv ? v[i] : 0.f, po, mo, vo);
                p[i] = po;
                if (m) m[i] = mo;
                if (v) v[i] = vo;
            }
            if (e) e[i] = ema(e[i], po);
        }
    }
}

template <int ALGO>
void opt_launch(bool has_ema, int blocks, hipStream_t stream, const hdy_opt_desc* table, int ndesc, const OptHyper& h) {
    if (has_ema) hipLaunchKernelGGL((opt_step_kernel<ALGO, true>), dim3(blocks), dim3(256), 0, stream, table, ndesc, h);
    else hipLaunchKernelGGL((opt_step_kernel<ALGO, false>), dim3(blocks), dim3(256), 0, stream, table, ndesc, h);
}

}  // namespace

extern "C" int hdy_opt_blocks(long long n) { return (int)((n + OPT_BLOCK_ELEMS - 1) / OPT_BLOCK_ELEMS); }

extern "C" int hdy_opt_step(const hdy_opt_desc* table_device, int ndesc, int total_blocks, int algo, int nesterov, const float* hyper, int nslots,
                            int has_ema, float ema_decay, float ema_one_minus_decay, void* stream) {
    HDY_ARG(table_device, "opt_step: null table");
    HDY_ARG(ndesc > 0 && total_blocks > 0, "opt_step: empty table (%d rows, %d blocks)", ndesc, total_blocks);
    HDY_ARG(algo == HDY_OPT_SGD || algo == HDY_OPT_ADAM || algo == HDY_OPT_ADAMW, "opt_step: unknown algorithm %d", algo);
    HDY_ARG(nslots >= 1 && nslots <= HDY_OPT_MAX_SLOTS, "opt_step: %d slots, 1..%d are served", nslots, HDY_OPT_MAX_SLOTS);
    HDY_ARG(hyper, "opt_step: null hyper-parameter array");
    OptHyper h = {};
    for (int i = 0; i < nslots * HDY_OPT_HYPER; ++i) h.v[i / HDY_OPT_HYPER][i % HDY_OPT_HYPER] = hyper[i];
    h.ema_d = ema_decay;
    h.ema_omd = ema_one_minus_decay;
    h.nesterov = nesterov;
    const hipStream_t s = (hipStream_t)stream;
    if (algo == HDY_OPT_SGD) opt_launch<HDY_OPT_SGD>(has_ema != 0, total_blocks, s, table_device, ndesc, h);
    else if (algo == HDY_OPT_ADAM) opt_launch<HDY_OPT_ADAM>(has_ema != 0, total_blocks, s, table_device, ndesc, h);
    else opt_launch<HDY_OPT_ADAMW>(has_ema != 0, total_blocks, s, table_device, ndesc, h);
    HDY_LAUNCH_CHECK("opt_step");
    return HDY_OK;
}
