// Internal (not part of the C ABI): argument blocks shared between the entry points (conv_dispatch.hip, api.hip) and the kernel files.
#pragma once
#include <type_traits>

#include "common.h"

// BatchNorm-backward statistics requested from the kernel that produces a gradient tensor (its LAST contribution): for the output
// channels [c0, c1) of the producer, which are the gradient dz of a Conv+BN+act unit's output, the epilogue also reads that unit's raw
// conv output y (same pixels; channel c0 of the producer = channel 0 of y/scale/...) and accumulates SUM du and SUM du*xhat per channel
// (du = dz * act'(y*scale + shift)) and SUM du*y into one fp32 slab [2][c1 - c0] per workgroup: slabs[wg][2][c1 - c0]; the finalize
// launch turns SUM du*y into SUM du*xhat = invstd * (SUM du*y - mean * SUM du), so the epilogue needs two coefficient vectors, not four.
struct StatReq {
    const void* y; int ldy;
    const float *scale, *shift;
    float* slabs;
    int c0, c1, act;
    int nslabs;           // slabs the caller's array holds (hdy_stat_req.nslabs)
};

struct ConvArgs {
    const void* x;        // [N][Hin][Win][ldx]
    const void* w;        // packed [Kpad][Kdp]
    void* y;              // [N][Hout][Wout][ldy]
    const float* scale;   // per-channel epilogue scale (or null = 1)
    const float* shift;   // per-channel epilogue shift / bias (or null = 0)
    float* stats;         // [stat_cap][2][K] BatchNorm partial sums (or null)
    int stat_cap;         // slabs the caller's `stats` array holds (hdy_conv_fwd's stat_slabs): checked against the slab count of the plan about to be
                          // launched (hdy_conv_take) — the sizing query and the launch both read the process-wide option table, which another
                          // thread may change in between
    const void* res;      // residual added after the activation, same pixel grid as y, pitch ldr (or null)
    int ldr;
    int N, Hin, Win, C, ldx;
    int Ho, Wo, K, ldy;
    int Hout, Wout, oh_mul, oh_off, ow_mul, ow_off;
    int ih_mul, iw_mul, dh0, dw0, TH, TW;
    int Kd, Kdp, M;
    int act, accumulate, dense_out;
    int mtiles, ntiles, bn;
    int span_pixels;      // 1: the C-wide read deliberately spans several ldx-pitched pixels (stem)
    int pointwise;        // derived: 1x1 stride-1 unpadded (input pixel == output pixel)
    int vec_out;          // derived: bf16 output rows can be written with 16-byte stores
    // Stride-2 dgrad as ONE launch: ncls = 4 parity classes of output pixels walked back to back per spatial tile (class = tile & 3).
    // Per class: tap window (c_TH x c_TW taps starting at dy offset c_dh / c_dw), k-blocks, output offsets, packed-weight offset (elements).
    // The scalar fields above (dh0, dw0, TH, TW, Kdp, oh_off, ow_off, w) hold class 0.  ncls <= 1: an ordinary launch.
    int nstat;            // 0..2 statistics requests served by the epilogue (dgrad, bf16 vector epilogue, single column tile)
    StatReq stat[2];
    int ncls;
    int c_dh[4], c_dw[4], c_TH[4], c_TW[4], c_nkb[4], c_oh[4], c_ow[4];
    long long c_w[4];
    // derived by hdy_conv_launch for the loader: union tap window over the classes (origin uh0 / uw0, UH x UW taps <= 31),
    // utap = every 128-byte k-block lies inside one tap (C % BKE == 0), reciprocals (hdy_magic) of Ho*Wo, Wo, C and the tap-window width
    int uh0, uw0, UH, UW, utap;
    int tile_interleave;  // 1: tiles that share A rows (column tiles of one m-tile, parity classes) go to neighbouring workgroups instead of one
    unsigned mg_howo, mg_wo, mg_c, mg_tw[4];
    int sh_howo, sh_wo, sh_c, sh_tw[4];
    int dbg;              // conv_deep.hip timing ablations (HDY_DEEP_DEBUG; results are wrong when set): 1 no A loads, 2 no B loads, 4 no MFMAs, 8 no epilogue, 16 no fragment reads
};

// ---- forward / data-gradient kernel selection -----------------------------------------------------------------------------------------
// The layer as the selection sees it, stated by every entry point that launches or sizes (conv_dispatch.hip: conv_shape for the forward
// pass; dgrad_shape, or one shape per parity class where a side is odd, for the data gradient: a convolution from dy's K channels to dx's C).
struct ConvShape {
    int N, H, W;          // input pixel grid (stem: the image, without its padding; data gradient: dy's)
    int Ho, Wo;           // output pixels per image the launch walks (ncls == 4: per parity class)
    int C, K, R, S, stride;   // ncls == 4: R, S, stride (2) and pad are those of the layer being DIFFERENTIATED (hdy_dgrad3x3s2_plan reads them; no
                          // other family reads R, S, pad, H or W of a class walk: conv_is is false for it and conv_taps is not asked)
    int pad;              // < 0: the window is not padded alike on both axes, or the output grid is not the one (H, W, R, S, stride, pad) give
    int dense;            // every output pixel is written (0: one parity class of a stride-2 data gradient)
    int dtype;
    int stem;             // the 6x6 / stride 2 / pad 2 stem on its 4-channel padded image (C == 3)
    int stats;            // the launch writes BatchNorm slabs (the sizing query asks with 1)
    int ncls;             // 4: the four-class walk of the stride-2 data gradient, else 1
};
// column tile of the generic kernel = row padding of a packed filter block
inline int hdy_conv_bn_tile(int K) { return K <= 32 ? 32 : (K <= 64 ? 64 : 128); }
inline int conv_out_dim(int in, int k, int stride, int pad) { return (in + 2 * pad - k) / stride + 1; }
// One spatial axis of a stride-2 dgrad parity class: output positions h = 2*i + a take the kernel taps
// r = rmax, rmax-2, ... (same parity as a + pad), reading dy row i + d0 + t for the t-th of them.
struct Axis { int taps, d0, rmax; };
inline Axis class_axis(int R, int pad, int a) {
    Axis ax = {0, 0, -1};
    for (int r = R - 1; r >= 0; --r)
        if (((a + pad - r) & 1) == 0) {
            if (ax.rmax < 0) { ax.rmax = r; ax.d0 = (a + pad - r) / 2; }
            ++ax.taps;
        }
    return ax;
}
// the layer hdy_conv_fwd / hdy_conv_stat_slabs are called with
inline ConvShape conv_shape(int N, int H, int W, int C, int K, int R, int S, int stride, int pad, int dtype, int stem, int stats) {
    return ConvShape{N, H, W, conv_out_dim(H, R, stride, pad), conv_out_dim(W, S, stride, pad), C, K, R, S, stride, pad, 1, dtype, stem, stats, 1};
}
inline long long conv_pixels(const ConvShape& s) { return (long long)s.N * s.Ho * s.Wo; }
inline int conv_taps(const ConvShape& s) { return s.stem ? 6 : s.R * s.S; }
// a square window with these parameters (then Ho, Wo follow from H, W)
inline bool conv_is(const ConvShape& s, int R, int stride, int pad) { return !s.stem && s.ncls <= 1 && s.R == R && s.S == R && s.stride == stride && s.pad == pad; }

// The order of this list is the order the families are asked in (conv_fwd_plan, conv_dispatch.hip); the generic kernel takes everything.
enum ConvFamily { CONV_NONE = 0, CONV_STEM, CONV_3X3_C64, CONV_3X3_C128, CONV_3X3S2, CONV_DGRAD_S2, CONV_DEEP, CONV_IGEMM };

// What one family answers for a shape: the sizing query reads `slabs`, the launch reads all of it.
struct ConvPlan {
    int family;           // ConvFamily
    int variant;          // the family's instance (input channels, planes, 256-row tile, ...)
    int grid;             // workgroups
    int slabs;            // statistic slabs a launch with `stats` writes
    int bn;               // column tile (deep-pipelined and generic kernel)
    int interleave;       // generic kernel: the HDY_TILE_INTERLEAVE value `slabs` was counted with (becomes ConvArgs.tile_interleave)
};

// <family>_plan: true = the shape is this family's, *p filled.  Pure host functions of the shape and the option table.
bool hdy_conv_stem_plan(const ConvShape& s, ConvPlan* p);
bool hdy_conv3x3_c64_plan(const ConvShape& s, ConvPlan* p);
bool hdy_conv3x3_c128_plan(const ConvShape& s, ConvPlan* p);
bool hdy_conv3x3s2_plan(const ConvShape& s, ConvPlan* p);
bool hdy_dgrad3x3s2_plan(const ConvShape& s, ConvPlan* p);
bool hdy_conv_deep_plan(const ConvShape& s, ConvPlan* p);
bool hdy_conv_igemm_plan(const ConvShape& s, ConvPlan* p);

// <family>_launch: starts the planned instance on the planned grid.  It decides nothing about the shape again; it checks what the shape
// cannot know (alignment, fp32 output, residual, accumulate, activation) and answers HDY_CONV_DECLINE when this call cannot run on it.
enum { HDY_CONV_DECLINE = -100 };
int hdy_conv_stem_launch(const ConvArgs& a, const ConvPlan& p, int out_f32, hipStream_t st);
int hdy_conv3x3_c64_launch(const ConvArgs& a, const ConvPlan& p, int out_f32, hipStream_t st);
int hdy_conv3x3_c128_launch(const ConvArgs& a, const ConvPlan& p, int out_f32, hipStream_t st);
int hdy_conv3x3s2_launch(const ConvArgs& a, const ConvPlan& p, int out_f32, hipStream_t st);
int hdy_dgrad3x3s2_launch(const ConvArgs& a, const ConvPlan& p, int out_f32, hipStream_t st);
int hdy_conv_deep_launch(const ConvArgs& a, const ConvPlan& p, int out_f32, hipStream_t st);
int hdy_conv_igemm_launch(const ConvArgs& a, const ConvPlan& p, int dtype, int out_f32, hipStream_t st);

// The one rule for a launch whose plan names a family.  `fits` = pointers, pitches and output type qualify for its kernel.  It does not
// fit: without statistics the next family in the order takes the launch; with statistics the caller sized the slab array with
// hdy_conv_stat_slabs for THIS family and any other kernel would write a different count, so that is an error.  It fits: the array must
// hold exactly what the plan writes (HDY_OK = go on and launch).
inline int hdy_conv_take(const ConvArgs& a, const ConvPlan& p, bool fits, const char* who) {
    if (!fits && !a.stats) return HDY_CONV_DECLINE;
    HDY_ARG(fits, "%s: statistics requested, but this call does not fit the kernel their slabs were sized for (bf16 output, 16-byte aligned x/y/res rows; "
            "ldx=%d ldy=%d)", who, a.ldx, a.ldy);
    HDY_ARG(!a.stats || a.stat_cap == p.slabs, "%s: the statistics array holds %d slabs, this launch writes %d (a kernel-selection option changed between "
            "hdy_conv_stat_slabs and the launch?)", who, a.stat_cap, p.slabs);
    return HDY_OK;
}

// x, y and the residual (need_w: the packed filter too) can be moved with 16-byte accesses
inline bool rows_aligned(const ConvArgs& a, bool need_w) {
    return a.ldx % 8 == 0 && a.ldy % 8 == 0 && (((uintptr_t)a.x | (uintptr_t)a.y) & 15) == 0 && (!need_w || (((uintptr_t)a.w & 15) == 0 && a.Kdp % 8 == 0)) &&
           (!a.res || (a.ldr % 8 == 0 && ((uintptr_t)a.res & 15) == 0));
}

// epilogue instance of the patch- and filter-resident kernels: 0 store, 1 scale / shift, 2 scale / shift + SiLU
inline int epilogue_of(const ConvArgs& a) { return a.act == 1 ? 2 : ((a.scale || a.shift) ? 1 : 0); }

// run-time (stats, epilogue) -> template arguments: f(std::bool_constant<STATS>, std::integral_constant<int, EPI>)
template <typename F> inline void with_stats_epi(bool stats, int epi, F&& f) {
    auto with_epi = [&](auto s) {
        if (epi == 2) f(s, std::integral_constant<int, 2>{});
        else if (epi == 1) f(s, std::integral_constant<int, 1>{});
        else f(s, std::integral_constant<int, 0>{});
    };
    if (stats) with_epi(std::true_type{});
    else with_epi(std::false_type{});
}

// status of the launch just issued
inline int hdy_launch_status(const char* who) {
    HDY_LAUNCH_CHECK(who);
    return HDY_OK;
}

// reciprocal for n / d, n < 2^31: q = mulhi(2n, *mg) >> *sh (conv_igemm.hip fdiv)
inline void hdy_magic(unsigned d, unsigned* mg, int* sh) {
    int s = 0;
    while ((1ull << s) < d) ++s;
    *mg = (unsigned)((((unsigned long long)1 << (31 + s)) + d - 1) / d);
    *sh = s;
}

struct WgradArgs {
    const void* x;        // [N][Hin][Win][ldx]
    const void* dy;       // [N][Ho][Wo][lddy]
    float* partial;       // [splits][K][Q]   Q = TH*TW*C
    int N, Hin, Win, C, ldx;
    int Ho, Wo, K, lddy;
    int ih_mul, iw_mul, dh0, dw0, TH, TW;
    int Q, P;             // Q = taps*C, P = N*Ho*Wo pixels
    int splits, pix_per_split;
    int ktiles, qtiles;
    int span_pixels;
    // stem kernel only: y != NULL = `dy` holds dz (gradient of the unit's activation output) and the kernel applies the BatchNorm / SiLU
    // backward itself while staging the tile: dy = scale * (dz * silu'(y*scale + shift) - c1 - (y - mean)*invstd * c2)
    const void* y; int ldy;
    const float *bn_scale, *bn_shift, *bn_mean, *bn_invstd, *bn_c1, *bn_c2;
};

// ---- weight-gradient kernel selection (same scheme as the forward side: shape -> plan in one walk, conv_dispatch.hip) ------------------
// The layer as hdy_conv_wgrad / hdy_conv_wgrad_workspace_bytes are called with it.
struct WgradShape {
    int N, H, W;          // input pixel grid (stem: the image, without its padding)
    int Ho, Wo;           // dy pixels per image
    int C, K, R, S, stride, pad, dtype;
    int stem;             // the 6x6 / stride 2 / pad 2 stem on its 4-channel padded image (C == 3)
};
inline WgradShape wgrad_shape(int N, int H, int W, int C, int K, int R, int S, int stride, int pad, int dtype, int stem) {
    return WgradShape{N, H, W, conv_out_dim(H, R, stride, pad), conv_out_dim(W, S, stride, pad), C, K, R, S, stride, pad, dtype, stem};
}
inline long long wgrad_pixels(const WgradShape& s) { return (long long)s.N * s.Ho * s.Wo; }
inline int wgrad_cols(const WgradShape& s) { return s.R * s.S * (s.stem ? 4 : s.C); }      // Q: columns of a slab [K][Q]

// The order of this list is the order the families are asked in (wgrad_plan, conv_dispatch.hip); the generic kernel takes everything.
enum WgradFamily { WGRAD_STEM, WGRAD_3X3, WGRAD_DEEP, WGRAD_GENERIC };

// What one family answers for a shape.  The launch writes `splits` slabs: splits * K * Q floats of workspace.
struct WgradPlan {
    int family;           // WgradFamily
    int variant;          // the family's instance (stem: K / 16; 3x3: 2 * (KB == 64) + (CB == 64); generic: 4 * fp32 + 2 * (SD == 2) + (SX == 2))
    int grid;             // workgroups
    int splits;           // slabs written
    int pix_per_split;    // generic and deep-pipelined kernel
    int ktiles, qtiles;   // tiles of the K x Q gradient (3x3: its KB x CB blocks)
    int TOH, TOW, tiles_h, tiles_w;      // 3x3: output tile and tiles per image
};

// <family>_plan: true = the shape is this family's, *p filled.  Pure host functions of the shape and the option table.
bool hdy_wgrad_stem_plan(const WgradShape& s, WgradPlan* p);
bool hdy_wgrad3x3_plan(const WgradShape& s, WgradPlan* p);
bool hdy_wgrad_deep_plan(const WgradShape& s, WgradPlan* p);
bool hdy_wgrad_generic_plan(const WgradShape& s, WgradPlan* p);

// <family>_launch: fills the family's argument block from the validated WgradArgs (hdy_conv_wgrad) and the plan and starts the planned
// instance.  Only the deep-pipelined kernel can answer HDY_CONV_DECLINE (its 31-bit offsets depend on the caller's pitches).
int hdy_wgrad_stem_launch(const WgradArgs& a, const WgradPlan& p, hipStream_t st);
int hdy_wgrad3x3_launch(const WgradArgs& a, const WgradPlan& p, hipStream_t st);
int hdy_wgrad_deep_launch(const WgradArgs& a, const WgradPlan& p, hipStream_t st);
int hdy_wgrad_generic_launch(const WgradArgs& a, const WgradPlan& p, hipStream_t st);
// grad_a [K_a][C][R][S] and the optional grad_b [K_b][C][R][S] (rows K_a.. of every slab) (+)= SUM over `splits` slabs [K][Q] (conv_wgrad.hip)
int hdy_wgrad_reduce(const float* partial, int splits, int K, int Q, int mode, int C, int R, int S, float* grad_a, int K_a, float* grad_b, int K_b,
                     int accumulate, hipStream_t st);
