// Kernel selection and launch of the convolution families (host code only).
//
// Forward / data gradient: conv_fwd_plan() is the one ordered walk over the families: each family's <name>_plan (in its own file) says
// whether a ConvShape is its own and, if so, with which instance, grid and statistic-slab count.  The sizing queries (hdy_conv_stat_slabs,
// hdy_conv_dgrad_stat_slabs) and the launch (hdy_conv_launch) below both read that plan, so the slab array a caller sized is the one the
// kernel about to start writes.  The entry points (hdy_conv_fwd, hdy_conv_dgrad, hdy_conv_dgrad_stats) follow: each states its layer as a
// ConvShape for the walk and as a ConvArgs (tap-window geometry) for the kernels.
//
// Weight gradient: the same with WgradShape / WgradPlan and wgrad_plan(); the workspace query (hdy_conv_wgrad_workspace_bytes) and the
// entry points that launch (hdy_conv_wgrad, hdy_conv_wgrad_stem_fused) are at the end of this file.
#include "common.h"
#include "hdyolo_internal.h"
#include "hdyolo.h"

static inline int bke(int dtype) { return dtype == HDY_BF16 ? 64 : 32; }      // elements of a 128-byte k-block

// the plan of the first family from `first` on that takes the shape
static ConvPlan conv_fwd_plan(const ConvShape& s, int first = CONV_STEM) {
    ConvPlan p = {};
    if (first <= CONV_STEM && hdy_conv_stem_plan(s, &p)) return p;                // patch-resident 6x6/s2 stem
    if (first <= CONV_3X3_C64 && hdy_conv3x3_c64_plan(s, &p)) return p;           // filter-resident 3x3, 32 / 64 input channels
    if (first <= CONV_3X3_C128 && hdy_conv3x3_c128_plan(s, &p)) return p;         // ... its 128-input-channel form
    if (first <= CONV_3X3S2 && hdy_conv3x3s2_plan(s, &p)) return p;               // patch-resident 3x3 / stride 2
    if (first <= CONV_DGRAD_S2 && hdy_dgrad3x3s2_plan(s, &p)) return p;           // ... its data gradient, 32 <- 64 and 64 <- 128 (four-class walk)
    if (first <= CONV_DEEP && hdy_conv_deep_plan(s, &p)) return p;                // deep-pipelined 256-row implicit GEMM (C % 64 == 0, K >= 128)
    hdy_conv_igemm_plan(s, &p);                                                   // generic implicit GEMM: takes everything
    return p;
}

extern "C" int hdy_conv_stat_slabs(int N, int H, int W, int C, int K, int R, int S, int stride, int pad, int dtype) {
    const int stem = C == 3 && R == 6 && S == 6 && stride == 2 && pad == 2;
    return conv_fwd_plan(conv_shape(N, H, W, C, K, R, S, stride, pad, dtype, stem, 1)).slabs;
}

static int launch_planned(const ConvArgs& a, const ConvPlan& p, int dtype, int out_f32, hipStream_t st) {
    switch (p.family) {
        case CONV_STEM: return hdy_conv_stem_launch(a, p, out_f32, st);
        case CONV_3X3_C64: return hdy_conv3x3_c64_launch(a, p, out_f32, st);
        case CONV_3X3_C128: return hdy_conv3x3_c128_launch(a, p, out_f32, st);
        case CONV_3X3S2: return hdy_conv3x3s2_launch(a, p, out_f32, st);
        case CONV_DGRAD_S2: return hdy_dgrad3x3s2_launch(a, p, out_f32, st);
        case CONV_DEEP: return hdy_conv_deep_launch(a, p, out_f32, st);
        default: return hdy_conv_igemm_launch(a, p, dtype, out_f32, st);
    }
}

// Host-side validation + dispatch shared by the entry points below: `s` is the layer `a` describes, as its caller states it.
static int hdy_conv_launch(ConvArgs a, const ConvShape& s, int out_f32, hipStream_t st) {
    const int dtype = s.dtype;
    const int VE = dtype == HDY_BF16 ? 8 : 4;
    HDY_ARG(a.x && a.w && a.y, "conv: null pointer");
    HDY_ARG(a.N > 0 && a.Hin > 0 && a.Win > 0 && a.Ho > 0 && a.Wo > 0 && a.K > 0 && a.C > 0, "conv: non-positive dim");
    HDY_ARG(a.C % VE == 0, "conv: C=%d must be a multiple of %d for this dtype", a.C, VE);
    HDY_ARG(a.ldx % (a.span_pixels ? 4 : VE) == 0 && (a.span_pixels || a.ldx >= a.C), "conv: ldx=%d must be >= C and a multiple of %d", a.ldx, VE);
    HDY_ARG(a.ldy >= a.K, "conv: ldy=%d < K=%d", a.ldy, a.K);
    HDY_ARG(((uintptr_t)a.x & 15) == 0 && ((uintptr_t)a.w & 15) == 0, "conv: x/w must be 16-byte aligned");
    HDY_ARG(a.TH > 0 && a.TW > 0, "conv: empty tap window");
    HDY_ARG(a.Hin < 24000 && a.Win < 24000 && a.TH < 64 && a.TW < 64 && a.dh0 > -4000 && a.dw0 > -4000, "conv: image side beyond the loader's 16-bit coordinates");
    HDY_ARG((long long)a.N * a.Hin * a.Win < (1LL << 31) && (long long)a.N * a.Ho * a.Wo < (1LL << 31), "conv: too many pixels");
    a.Kd = a.TH * a.TW * a.C;
    const int BKE = 8 * VE;
    a.bn = hdy_conv_bn_tile(a.K);
    HDY_ARG(a.Kdp == round_up(a.Kd, BKE), "conv: packed weight pitch %d != %d", a.Kdp, round_up(a.Kd, BKE));
    a.M = a.N * a.Ho * a.Wo;
    a.mtiles = cdiv(a.M, 128);
    a.ntiles = cdiv(a.K, a.bn);
    if (a.dense_out) HDY_ARG(a.oh_mul == 1 && a.ow_mul == 1 && a.oh_off == 0 && a.ow_off == 0 && a.Hout == a.Ho && a.Wout == a.Wo, "conv: dense_out geometry mismatch");
    // 1x1 / stride 1 / no padding: input pixel == output pixel, no coordinate arithmetic in the loader
    a.pointwise = (a.TH == 1 && a.TW == 1 && a.ih_mul == 1 && a.iw_mul == 1 && a.dh0 == 0 && a.dw0 == 0 && a.Hin == a.Ho && a.Win == a.Wo &&
                   !a.span_pixels && a.ncls <= 1) ? 1 : 0;
    if (a.ncls > 1) {
        HDY_ARG(a.ncls == 4 && !a.dense_out && !a.stats, "conv: class walk is the four-class stride-2 dgrad");
        for (int c = 0; c < 4; ++c) HDY_ARG(a.c_nkb[c] == round_up(a.c_TH[c] * a.c_TW[c] * a.C, BKE) / BKE, "conv: class %d k-blocks", c);
    }
    // coalesced 16-byte epilogue needs bf16 output, whole vectors and aligned rows
    const bool bf16_out = dtype == HDY_BF16 && !out_f32;
    a.vec_out = (bf16_out && a.K % 8 == 0 && a.ldy % 8 == 0 && ((uintptr_t)a.y & 15) == 0 &&
                 (!a.res || (a.ldr % 8 == 0 && ((uintptr_t)a.res & 15) == 0))) ? 1 : 0;
    if (a.nstat > 0) {
        HDY_ARG(a.nstat <= 2 && a.vec_out && a.ntiles == 1 && a.bn <= 64 && !a.stats && !a.res, "conv: producer-side statistics need the bf16 vector epilogue and at most 64 output channels");
        for (int r = 0; r < a.nstat; ++r) {
            const StatReq& q = a.stat[r];
            HDY_ARG(q.y && q.scale && q.shift && q.slabs && q.c0 >= 0 && q.c0 < q.c1 && q.c1 <= a.K && q.c0 % 8 == 0 && q.c1 % 8 == 0 &&
                    q.ldy % 8 == 0 && (((uintptr_t)q.y | (uintptr_t)q.scale | (uintptr_t)q.shift) & 15) == 0,
                    "conv: bad statistics request %d", r);
        }
    }
    // loader geometry: union tap window over the classes, reciprocals for the row / chunk decompositions
    a.uh0 = a.dh0; a.uw0 = a.dw0;
    int uh1 = a.dh0 + a.TH, uw1 = a.dw0 + a.TW;
    for (int c = 0; c < (a.ncls > 1 ? 4 : 0); ++c) {
        a.uh0 = a.c_dh[c] < a.uh0 ? a.c_dh[c] : a.uh0; a.uw0 = a.c_dw[c] < a.uw0 ? a.c_dw[c] : a.uw0;
        uh1 = a.c_dh[c] + a.c_TH[c] > uh1 ? a.c_dh[c] + a.c_TH[c] : uh1; uw1 = a.c_dw[c] + a.c_TW[c] > uw1 ? a.c_dw[c] + a.c_TW[c] : uw1;
    }
    a.UH = uh1 - a.uh0; a.UW = uw1 - a.uw0;
    HDY_ARG(a.UH * a.UW <= 31, "conv: %d x %d tap window beyond the loader's 31 tap bits", a.UH, a.UW);
    HDY_ARG(((long long)(a.UH + 1) * a.Win + a.UW) * a.ldx * (dtype == HDY_BF16 ? 2 : 4) < (1LL << 28), "conv: tap window spans too many bytes");
    // The loader's per-row offsets are unsigned, from the window origin of the tile's FIRST row.  Where an output row is more than one pixel
    // wider than what it reads (pad > S / 2, or the data gradient of a layer padded by less than (S - 1) / 2), or likewise taller, a later
    // row's origin lies BEFORE the first one's.  The per-lane form adds the tap to the offset in 32 bits, which wraps back into range; the
    // whole-tap form hands the tap to the descriptor as a scalar offset, and the range check then drops every tap of such a row (zeros).
    const bool ascending = (long long)(a.Wo - 1) * a.iw_mul <= a.Win && (long long)(a.Ho - 1) * a.ih_mul < a.Hin;
    a.utap = (a.C % BKE == 0 && ascending) ? 1 : 0;
    hdy_magic((unsigned)(a.Ho * a.Wo), &a.mg_howo, &a.sh_howo);
    hdy_magic((unsigned)a.Wo, &a.mg_wo, &a.sh_wo);
    hdy_magic((unsigned)a.C, &a.mg_c, &a.sh_c);
    for (int c = 0; c < 4; ++c) hdy_magic((unsigned)(a.ncls > 1 ? a.c_TW[c] : a.TW), &a.mg_tw[c], &a.sh_tw[c]);
    // Producer-side statistics (nstat) exist in the generic kernel only.  A family whose plan it is but whose kernel this call does not
    // fit (hdy_conv_take) hands the launch to the families after it.
    for (int first = a.nstat > 0 ? CONV_IGEMM : CONV_STEM;;) {
        const ConvPlan p = conv_fwd_plan(s, first);
        a.tile_interleave = p.interleave;
        const int rc = launch_planned(a, p, dtype, out_f32, st);
        if (rc != HDY_CONV_DECLINE) return rc;
        first = p.family + 1;
    }
}

// ---- data gradient --------------------------------------------------------------------------------------------------------------------
// Stride-2 data gradient as ONE launch that walks the four parity classes per spatial tile: every class has the same Ho x Wo (even H and W)
// and taps of its own.
static bool dgrad_class_walk(int H, int W, int R, int S, int pad) {
    if (H % 2 || W % 2 || hdy_opt(HDY_OPT_NO_CLASS_WALK)) return false;
    for (int a = 0; a < 2; ++a)
        if (!class_axis(R, pad, a).taps || !class_axis(S, pad, a).taps) return false;
    return true;
}

// The data gradient of a layer as the convolution from dy's K channels, on dy's pixel grid, to dx's C.  Stride 1: the same window with
// pad' = R - 1 - pad (-1 where no forward window has that padding).  Stride 2, where dgrad_class_walk holds: the four-class walk over
// H/2 x W/2 pixels per class, with the window of the layer being differentiated (hdyolo_internal.h, ConvShape).
static ConvShape dgrad_shape(int N, int H, int W, int C, int K, int R, int S, int stride, int pad, int dtype) {
    const bool walk = stride == 2;
    const int pad1 = R == S && pad <= R - 1 ? R - 1 - pad : -1;
    return ConvShape{N, conv_out_dim(H, R, stride, pad), conv_out_dim(W, S, stride, pad), H / stride, W / stride, K, C, R, S, stride, walk ? pad : pad1,
                     !walk, dtype, 0, 0, walk ? 4 : 1};
}

// dx (+)= conv_transpose(dy, w): dx is [N][H][W][lddx] (C channels), dy is [N][Ho][Wo][lddy] (K channels).
static int dgrad_impl(const void* dy, int lddy, const void* w_packed_dgrad, void* dx, int lddx, int N, int H, int W, int C, int K, int R,
                      int S, int stride, int pad, int accumulate, int dtype, const hdy_stat_req* stats, int nstat, void* stream) {
    HDY_ARG(stride == 1 || stride == 2, "conv_dgrad: stride %d unsupported", stride);
    HDY_ARG(dtype == HDY_BF16 || dtype == HDY_F32, "conv_dgrad: unknown dtype %d", dtype);
    const int Ho = conv_out_dim(H, R, stride, pad), Wo = conv_out_dim(W, S, stride, pad);
    HDY_ARG(Ho > 0 && Wo > 0, "conv_dgrad: empty dy");
    ConvArgs a = {};
    a.x = dy; a.y = dx; a.N = N; a.Hin = Ho; a.Win = Wo; a.C = K; a.ldx = lddy;
    a.K = C; a.ldy = lddx; a.Hout = H; a.Wout = W;
    a.ih_mul = a.iw_mul = 1; a.accumulate = accumulate;
    a.nstat = nstat;
    for (int r = 0; r < nstat; ++r)
        a.stat[r] = StatReq{stats[r].y, stats[r].ldy, stats[r].scale, stats[r].shift, stats[r].slabs, stats[r].c0, stats[r].c1, stats[r].act, stats[r].nslabs};
    if (stride == 1) {
        a.w = w_packed_dgrad;
        a.Ho = H; a.Wo = W; a.oh_mul = a.ow_mul = 1; a.dense_out = 1;
        a.dh0 = pad - (R - 1); a.dw0 = pad - (S - 1); a.TH = R; a.TW = S;
        a.Kdp = round_up(R * S * K, bke(dtype));
        return hdy_conv_launch(a, dgrad_shape(N, H, W, C, K, R, S, stride, pad, dtype), 0, (hipStream_t)stream);
    }
    // checked for both axes before anything starts: found inside the loop of launches below, the classes before the empty one had already
    // written their pixels of dx when the call failed
    for (int ca = 0; ca < 2; ++ca)
        HDY_ARG(class_axis(R, pad, ca).taps && class_axis(S, pad, ca).taps,
                "conv_dgrad: kernel %dx%d pad %d leaves a parity class without taps (unsupported)", R, S, pad);
    const int rows_total = round_up(C, hdy_conv_bn_tile(C));
    size_t off = 0;
    // One launch walking the four parity classes per spatial tile (conv_igemm.hip, `walk`): every class has the same Ho x Wo when H and W
    // are even.  As four launches each class wrote every other pixel of every other row (half cache lines, each line written by two
    // launches) and read dy from HBM again: 32<-64 @320x320 B=64 took 353 us against a 100 us bound.
    if (dgrad_class_walk(H, W, R, S, pad)) {
        ConvArgs c = a;
        c.ncls = 4;
        c.Ho = H / 2; c.Wo = W / 2;
        c.oh_mul = c.ow_mul = 2; c.dense_out = 0;
        for (int ca = 0; ca < 2; ++ca)
            for (int cb = 0; cb < 2; ++cb) {
                const Axis ah = class_axis(R, pad, ca), aw = class_axis(S, pad, cb);
                const int i = ca * 2 + cb;
                const int Kdp = round_up(ah.taps * aw.taps * K, bke(dtype));
                c.c_dh[i] = ah.d0; c.c_dw[i] = aw.d0; c.c_TH[i] = ah.taps; c.c_TW[i] = aw.taps;
                c.c_nkb[i] = Kdp / bke(dtype); c.c_oh[i] = ca; c.c_ow[i] = cb; c.c_w[i] = (long long)off;
                off += (size_t)rows_total * Kdp;
            }
        c.w = w_packed_dgrad;
        c.dh0 = c.c_dh[0]; c.dw0 = c.c_dw[0]; c.TH = c.c_TH[0]; c.TW = c.c_TW[0]; c.oh_off = c.ow_off = 0;
        c.Kdp = c.c_nkb[0] * bke(dtype);
        return hdy_conv_launch(c, dgrad_shape(N, H, W, C, K, R, S, stride, pad, dtype), 0, (hipStream_t)stream);
    }
    for (int ca = 0; ca < 2; ++ca)
        for (int cb = 0; cb < 2; ++cb) {
            const Axis ah = class_axis(R, pad, ca), aw = class_axis(S, pad, cb);
            ConvArgs c = a;
            c.Ho = (H - ca + 1) / 2; c.Wo = (W - cb + 1) / 2;
            c.oh_mul = c.ow_mul = 2; c.oh_off = ca; c.ow_off = cb; c.dense_out = 0;
            if (c.Ho <= 0 || c.Wo <= 0) continue;
            c.dh0 = ah.d0; c.dw0 = aw.d0; c.TH = ah.taps; c.TW = aw.taps;
            c.Kdp = round_up(ah.taps * aw.taps * K, bke(dtype));
            c.w = (const char*)w_packed_dgrad + off * (dtype == HDY_BF16 ? 2 : 4);
            off += (size_t)rows_total * c.Kdp;
            // one parity class alone: its own tap window at stride 1, no padding a forward window has; only the implicit-GEMM families take it
            const ConvShape s = {N, Ho, Wo, c.Ho, c.Wo, K, C, ah.taps, aw.taps, 1, -1, 0, dtype, 0, 0, 1};
            const int rc = hdy_conv_launch(c, s, 0, (hipStream_t)stream);
            if (rc) return rc;
        }
    return HDY_OK;
}

extern "C" {

// y = act(scale * conv(x, w) + shift) [+= y]; NHWC with pixel pitches; optional BatchNorm slabs in `stats`.
// stem != 0: x is the hdy_stem_prep() buffer [N][H+2*pad][W+2*pad][4] and (C,R,S,stride,pad) must be (3,6,6,2,2).
int hdy_conv_fwd(const void* x, int ldx, const void* w_packed, const float* scale, const float* shift, const void* res, int ldr, void* y,
                 int ldy, float* stats, int stat_slabs, int N, int H, int W, int C, int K, int R, int S, int stride, int pad, int act, int accumulate,
                 int dtype, int out_f32, int stem, void* stream) {
    HDY_ARG(!stats || stat_slabs > 0, "conv_fwd: stats given with stat_slabs = %d", stat_slabs);
    HDY_ARG(stride >= 1 && R >= 1 && S >= 1 && pad >= 0, "conv_fwd: bad window");
    HDY_ARG(dtype == HDY_BF16 || dtype == HDY_F32, "conv_fwd: unknown dtype %d", dtype);
    ConvArgs a = {};
    a.x = x; a.w = w_packed; a.y = y; a.scale = scale; a.shift = shift; a.stats = stats; a.stat_cap = stat_slabs; a.res = res; a.ldr = ldr;
    HDY_ARG(!res || ldr >= K, "conv_fwd: residual pitch %d < K", ldr);
    a.N = N;
    a.Ho = conv_out_dim(H, R, stride, pad);
    a.Wo = conv_out_dim(W, S, stride, pad);
    HDY_ARG(a.Ho > 0 && a.Wo > 0, "conv_fwd: empty output");
    a.K = K; a.ldy = ldy;
    a.Hout = a.Ho; a.Wout = a.Wo; a.oh_mul = a.ow_mul = 1; a.oh_off = a.ow_off = 0; a.dense_out = 1;
    a.act = act; a.accumulate = accumulate;
    if (stem) {
        HDY_ARG(C == 3 && R == 6 && S == 6 && stride == 2 && pad == 2 && ldx == 4, "conv_fwd: stem expects C=3 k=6 s=2 p=2 on a 4-channel padded image");
        a.Hin = H + 2 * pad; a.Win = W + 2 * pad; a.C = 24; a.ldx = 4; a.span_pixels = 1;
        a.ih_mul = 2; a.iw_mul = 2; a.dh0 = 0; a.dw0 = 0; a.TH = 6; a.TW = 1;
        a.Kdp = round_up(6 * 24, bke(dtype));
    } else {
        a.Hin = H; a.Win = W; a.C = C; a.ldx = ldx;
        a.ih_mul = stride; a.iw_mul = stride; a.dh0 = -pad; a.dw0 = -pad; a.TH = R; a.TW = S;
        a.Kdp = round_up(R * S * C, bke(dtype));
    }
    return hdy_conv_launch(a, conv_shape(N, H, W, C, K, R, S, stride, pad, dtype, stem != 0, stats != nullptr), out_f32, (hipStream_t)stream);
}

int hdy_conv_dgrad(const void* dy, int lddy, const void* w_packed_dgrad, void* dx, int lddx, int N, int H, int W, int C, int K, int R,
                   int S, int stride, int pad, int accumulate, int dtype, void* stream) {
    return dgrad_impl(dy, lddy, w_packed_dgrad, dx, lddx, N, H, W, C, K, R, S, stride, pad, accumulate, dtype, nullptr, 0, stream);
}

int hdy_conv_dgrad_stats(const void* dy, int lddy, const void* w_packed_dgrad, void* dx, int lddx, int N, int H, int W, int C, int K, int R,
                         int S, int stride, int pad, int accumulate, int dtype, const hdy_stat_req* stats, int nstat, void* stream) {
    HDY_ARG(nstat >= 0 && nstat <= 2 && (nstat == 0 || stats), "conv_dgrad_stats: bad request count");
    HDY_ARG(nstat == 0 || hdy_conv_dgrad_stat_slabs(N, H, W, C, K, R, S, stride, pad, dtype) > 0, "conv_dgrad_stats: this shape cannot serve statistics");
    return dgrad_impl(dy, lddy, w_packed_dgrad, dx, lddx, N, H, W, C, K, R, S, stride, pad, accumulate, dtype, stats, nstat, stream);
}

// workgroups of the data-gradient launch that would serve statistics: stride 1, or stride 2 as ONE class-walking launch.  The statistics
// instances are the generic kernel's with at most 64 output channels (the 128-wide ones have no registers to spare for the operands).
int hdy_conv_dgrad_stat_slabs(int N, int H, int W, int C, int K, int R, int S, int stride, int pad, int dtype) {
    if (dtype != HDY_BF16 || C % 8 || hdy_conv_bn_tile(C) > 64 || (stride != 1 && stride != 2)) return 0;
    if (stride == 2 && !dgrad_class_walk(H, W, R, S, pad)) return 0;
    return conv_fwd_plan(dgrad_shape(N, H, W, C, K, R, S, stride, pad, dtype), CONV_IGEMM).grid;
}

}  // extern "C"

// ---- weight gradient ------------------------------------------------------------------------------------------------------------------
// the plan of the first family from `first` on that takes the shape
static WgradPlan wgrad_plan(const WgradShape& s, int first = WGRAD_STEM) {
    WgradPlan p = {};
    if (first <= WGRAD_STEM && hdy_wgrad_stem_plan(s, &p)) return p;              // patch-resident 6x6/s2 stem
    if (first <= WGRAD_3X3 && hdy_wgrad3x3_plan(s, &p)) return p;                 // patch-resident 3x3 / stride 1
    if (first <= WGRAD_DEEP && hdy_wgrad_deep_plan(s, &p)) return p;              // deep-pipelined 256 x 256 tiles (multi-tap, C % 64 == 0, K >= 192)
    hdy_wgrad_generic_plan(s, &p);                                                // generic kernel: takes everything
    return p;
}

static int wgrad_launch_planned(const WgradArgs& a, const WgradPlan& p, hipStream_t st) {
    switch (p.family) {
        case WGRAD_STEM: return hdy_wgrad_stem_launch(a, p, st);
        case WGRAD_3X3: return hdy_wgrad3x3_launch(a, p, st);
        case WGRAD_DEEP: return hdy_wgrad_deep_launch(a, p, st);
        default: return hdy_wgrad_generic_launch(a, p, st);
    }
}

// The kernels' view of the layer: the tap window over x, the stem as six row taps over the 24 pseudo channels of its padded 4-channel image.
static WgradArgs wgrad_args(const WgradShape& s, const void* x, int ldx, const void* dy, int lddy, void* workspace) {
    WgradArgs a = {};
    a.x = x; a.dy = dy; a.partial = (float*)workspace;
    a.N = s.N; a.K = s.K; a.lddy = lddy; a.Ho = s.Ho; a.Wo = s.Wo;
    if (s.stem) {
        a.Hin = s.H + 2 * s.pad; a.Win = s.W + 2 * s.pad; a.C = 24; a.ldx = 4; a.span_pixels = 1;
        a.ih_mul = a.iw_mul = 2; a.dh0 = a.dw0 = 0; a.TH = 6; a.TW = 1;
    } else {
        a.Hin = s.H; a.Win = s.W; a.C = s.C; a.ldx = ldx;
        a.ih_mul = a.iw_mul = s.stride; a.dh0 = a.dw0 = -s.pad; a.TH = s.R; a.TW = s.S;
    }
    return a;
}

// What every weight-gradient kernel needs of a call, checked once; then the planned family (one that declines hands the launch to the
// families after it) and the reduction of its slabs.  a.y set (the stem's fused BatchNorm backward): the caller has asked the stem's plan.
static int wgrad_run(const WgradShape& s, const WgradArgs& a, float* grad_a, int K_a, float* grad_b, int K_b, int accumulate, size_t ws_bytes, hipStream_t st) {
    const int VE = s.dtype == HDY_BF16 ? 8 : 4;
    HDY_ARG(grad_a && K_a > 0 && K_a + K_b <= a.K && K_b >= 0 && (K_b == 0) == (grad_b == nullptr), "wgrad: bad gradient split");
    HDY_ARG(a.x && a.dy && a.partial, "wgrad: null pointer");
    HDY_ARG(a.C % VE == 0 && a.K % VE == 0, "wgrad: C=%d and K=%d must be multiples of %d", a.C, a.K, VE);
    HDY_ARG(a.ldx % (a.span_pixels ? 4 : VE) == 0 && a.lddy % VE == 0 && (a.span_pixels || a.ldx >= a.C) && a.lddy >= a.K, "wgrad: bad pitches ldx=%d lddy=%d", a.ldx, a.lddy);
    HDY_ARG(((uintptr_t)a.x & 15) == 0 && ((uintptr_t)a.dy & 15) == 0, "wgrad: x/dy must be 16-byte aligned");
    HDY_ARG((long long)a.N * a.Hin * a.Win < (1LL << 31) && (long long)a.N * a.Ho * a.Wo < (1LL << 31), "wgrad: too many pixels");
    HDY_ARG(ws_bytes >= hdy_conv_wgrad_workspace_bytes(s.N, s.H, s.W, s.C, s.K, s.R, s.S, s.stride, s.pad, s.dtype, s.stem), "wgrad: workspace too small");
    WgradPlan p;
    int rc;
    for (int first = WGRAD_STEM;; first = p.family + 1) {
        p = wgrad_plan(s, first);
        rc = wgrad_launch_planned(a, p, st);
        if (rc != HDY_CONV_DECLINE) break;
    }
    if (rc) return rc;
    return hdy_wgrad_reduce(a.partial, p.splits, s.K, wgrad_cols(s), s.stem, s.C, s.R, s.S, grad_a, K_a, grad_b, K_b, accumulate, st);
}

extern "C" {

// The maximum over the plans of ALL families that take the shape, not the first one's: a call that does not fit its planned kernel (the
// deep-pipelined kernel's offset bound depends on the caller's pitches) falls to a later family and must find room for that one's slabs.
size_t hdy_conv_wgrad_workspace_bytes(int N, int H, int W, int C, int K, int R, int S, int stride, int pad, int dtype, int stem) {
    const WgradShape s = wgrad_shape(N, H, W, C, K, R, S, stride, pad, dtype, stem);
    int splits = 0;
    for (int first = WGRAD_STEM; first <= WGRAD_GENERIC;) {
        const WgradPlan p = wgrad_plan(s, first);
        if (p.splits > splits) splits = p.splits;
        first = p.family + 1;
    }
    return (size_t)splits * K * wgrad_cols(s) * sizeof(float);
}

// grad_a [K_a][C][R][S] (and optionally grad_b [K_b][C][R][S], the lower rows of a stacked weight) (+)= dW.
int hdy_conv_wgrad(const void* x, int ldx, const void* dy, int lddy, int N, int H, int W, int C, int K, int R, int S, int stride, int pad,
                   float* grad_a, int K_a, float* grad_b, int K_b, int accumulate, void* workspace, size_t ws_bytes, int dtype, int stem,
                   void* stream) {
    HDY_ARG(dtype == HDY_BF16 || dtype == HDY_F32, "conv_wgrad: unknown dtype %d", dtype);
    const WgradShape s = wgrad_shape(N, H, W, C, K, R, S, stride, pad, dtype, stem != 0);
    HDY_ARG(s.Ho > 0 && s.Wo > 0, "conv_wgrad: empty dy");
    HDY_ARG(!stem || (C == 3 && R == 6 && S == 6 && stride == 2 && pad == 2 && ldx == 4), "conv_wgrad: stem expects C=3 k=6 s=2 p=2 on a 4-channel padded image");
    return wgrad_run(s, wgrad_args(s, x, ldx, dy, lddy, workspace), grad_a, K_a, grad_b, K_b, accumulate, ws_bytes, (hipStream_t)stream);
}

// The stem's weight gradient with the BatchNorm / SiLU backward of its unit applied while the tile is staged (conv_wgrad.hip,
// wgrad_stem_kernel<.., true>): dz = gradient of the unit's output, y = its raw conv output, c1 / c2 from the statistics pass
// (hdy_bn_act_bwd with dy == NULL).  The stem has no data gradient, so dy is never materialised.  bf16, K in {16, 32, 64}: the stem
// family's plan, launched with the fused operands set.
int hdy_conv_wgrad_stem_fused_ok(int N, int H, int W, int K) {
    WgradPlan p;
    return (K == 16 || K == 32 || K == 64) && hdy_wgrad_stem_plan(wgrad_shape(N, H, W, 3, K, 6, 6, 2, 2, HDY_BF16, 1), &p);
}

int hdy_conv_wgrad_stem_fused(const void* x, const void* dz, int lddz, const void* y, int ldy, const float* scale, const float* shift, const float* mean,
                              const float* invstd, const float* c1, const float* c2, int N, int H, int W, int K, float* grad_a, int K_a, float* grad_b,
                              int K_b, int accumulate, void* workspace, size_t ws_bytes, void* stream) {
    HDY_ARG(y, "conv_wgrad_stem_fused: null pointer");
    HDY_ARG(hdy_conv_wgrad_stem_fused_ok(N, H, W, K), "conv_wgrad_stem_fused: shape not served (K in {16, 32, 64}, output a multiple of 16 x 32)");
    const WgradShape s = wgrad_shape(N, H, W, 3, K, 6, 6, 2, 2, HDY_BF16, 1);
    WgradArgs a = wgrad_args(s, x, 4, dz, lddz, workspace);
    a.y = y; a.ldy = ldy; a.bn_scale = scale; a.bn_shift = shift; a.bn_mean = mean; a.bn_invstd = invstd; a.bn_c1 = c1; a.bn_c2 = c2;
    return wgrad_run(s, a, grad_a, K_a, grad_b, K_b, accumulate, ws_bytes, (hipStream_t)stream);
}

}  // extern "C"
