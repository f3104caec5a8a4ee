/* hdyolo.h — C ABI of libhdyolo_hip.so: the MI355X (gfx950) kernels behind hd_yolo's metayolo detection hot path.
 *
 * The reference (impromptuRong/hd_yolo) is pure Python on PyTorch: it has no FFI / plugin registry.  The native
 * boundary of its hot path is wherever ATen / torchvision are entered, so each entry point below names the
 * reference call site whose native work it replaces (paths relative to the reference repo root).
 * INTEGRATION.md shows the ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *  - Plain pointers and sizes only; every buffer (inputs, outputs, workspaces) is owned by the caller.
 *    The library allocates nothing, keeps no pointers after a call returns and never synchronises.
 *  - All work is enqueued on `stream` (a hipStream_t passed as void*; NULL = the null stream).
 *  - Return value: 0 = ok; < 0 = invalid argument / unsupported shape; > 0 = a hipError_t from the launch.
 *    hdy_last_error() returns a thread-local description of the last failure.  Re-entrant.  Process state is limited to: the
 *    option table (atomics, initialised once from the environment under std::call_once, changed by hdy_set_option), per-kernel
 *    once-flags for the "dynamic LDS size" function attribute, and the thread-local error text / dispatch log.
 *  - Activations are NHWC ("channels last") with an explicit pixel pitch `ld*` in ELEMENTS, so a tensor may be
 *    a channel slice of a wider buffer (this is how torch.cat along C costs nothing).  Framework weights stay
 *    in the reference layout [K][C][R][S] fp32 and are re-packed by hdy_conv_pack.
 *  - dtype: HDY_F32 (exact fp32 MFMA, parity mode) or HDY_BF16 (bf16 operands, fp32 accumulate).  Per-channel
 *    vectors (scale/shift/statistics/gradients of them) are always fp32.
 *  - Alignment: activation and packed-weight pointers 16 bytes; channel counts and pitches multiples of one
 *    16-byte vector (8 bf16 / 4 f32) unless stated otherwise.
 */
#ifndef HDYOLO_H
#define HDYOLO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HDY_F32 0
#define HDY_BF16 1

#define HDY_PACK_FWD 0   /* operand of hdy_conv_fwd / layout of hdy_conv_wgrad results */
#define HDY_PACK_DGRAD 1 /* operand of hdy_conv_dgrad */
#define HDY_PACK_STEM 2  /* operand of hdy_conv_fwd(stem=1) */

#define HDY_ACT_NONE 0
#define HDY_ACT_SILU 1
#define HDY_ACT_RELU 2 /* the Mask-RCNN head's convolutions (row f2) */

const char* hdy_last_error(void);
/* ABI revision of THIS header: bumped whenever an entry point's parameter list, a structure or an option changes meaning.  hdy_version() returns the
 * value the library was built with; a binding written against another revision must refuse the library (hd_yolo_amd/_lib.py:load does) — with
 * plain pointers and sizes a mismatched parameter list would otherwise shift arguments silently. */
#define HDY_ABI_VERSION 15
int hdy_version(void);
/* Which kernel ran: every launcher names the kernel family it picked ("igemm_128x128x2", "conv3x3_c64", "deep_256x128", "wgrad3x3", ...;
 * hdy_sppf_pool_fwd: "sppf_fwd_keys32" / "_keys16" / "_float32" / "_float16" / "_c8", with "_pos" appended when positions are stored;
 * hdy_sppf_pool_bwd: "sppf_bwd_c16" / "sppf_bwd_c8_two" / "sppf_bwd_c8_one").
 * hdy_last_dispatch: the last pick on this thread; hdy_dispatch_log: every pick of every thread since hdy_dispatch_log_reset(), in launch
 * order, ';'-separated (process-wide under a mutex — autograd runs the backward list on its own thread — first 32 KB).  The reference has no counterpart (ATen picks its kernels silently); the tests use it to assert that the shapes meant to hit
 * a specialised kernel do. */
const char* hdy_last_dispatch(void);
const char* hdy_dispatch_log(void);
void hdy_dispatch_log_reset(void);
/* Process-wide kernel-selection switches by the name of their environment variable (HDY_NO_CONV3X3, HDY_NO_DEEP, HDY_WGRAD_BLOCKS, ...:
 * csrc/common.h HdyOption).  hdy_set_option returns the previous value (< 0: unknown name).  They also steer the sizing queries, so set
 * them before sizing buffers / building plans. */
int hdy_set_option(const char* name, int value);
int hdy_get_option(const char* name);
/* host-only: the reciprocal conv_igemm.hip divides row indices by (n / d == mulhi(2n, *magic) >> *shift for n < 2^31) */
int hdy_fastdiv_magic(unsigned d, unsigned* magic, int* shift);

/* ---- convolution family --------------------------------------------------------------------------------------
 * Replaces nn.Conv2d forward/backward as used by metayolo/models/layers.py:31,37-41 (Conv), :92-97 (Bottleneck),
 * :124-131 (C3), :179-189 (SPPF) and metayolo/models/yolo_head.py:112,142 (Detect's 1x1 conv with bias);
 * backward is what train.py:472 `scaler.scale(loss).backward()` reaches through autograd. */
int hdy_conv_out_dim(int in, int k, int stride, int pad);
int hdy_conv_mtiles(long long M); /* upper bound of the statistic slab count: one per 128 output pixels */
/* Number of [2][K] BatchNorm statistic slabs hdy_conv_fwd writes for this layer (kernel-dependent: one per 128 output pixels in
 * the generic kernel, one per workgroup in the filter-resident 3x3 kernel).  hdy_bn_finalize takes the same number. */
int hdy_conv_stat_slabs(int N, int H, int W, int C, int K, int R, int S, int stride, int pad, int dtype);

size_t hdy_conv_pack_elems(int K, int C, int R, int S, int stride, int pad, int kind, int dtype);
/* Logical weight [K][C][R][S] = rows of w_a, then rows of w_b (two convs fused along K; may be NULL/0), then zero rows up to K. */
int hdy_conv_pack(const float* w_a, int K_a, const float* w_b, int K_b, int K, int C, int R, int S, int stride, int pad, int kind,
                  int dtype, void* out, void* stream);

/* Batched packing: one launch re-packs every layer's weights after an optimizer step.  hdy_conv_pack_describe fills 1 (or 4:
 * stride-2 dgrad parity classes) descriptors on the HOST for the same arguments as hdy_conv_pack and returns how many it wrote
 * (first_block = running block count of the batch; each descriptor reports its nblocks); the caller copies all descriptors into
 * device memory once and replays hdy_conv_pack_run(table, n, total_blocks) every step. */
typedef struct hdy_pack_desc {
    const float* w_a;
    const float* w_b;
    void* out;
    int K_a, K_b, Kl, C, R, S, transpose, TH, TW, rbase, rstep, sbase, sstep, stem, rows_total, Kdp, dtype;
    int first_block, nblocks;
    int pad_;
} hdy_pack_desc;
int hdy_conv_pack_describe(const float* w_a, int K_a, const float* w_b, int K_b, int K, int C, int R, int S, int stride, int pad, int kind,
                           int dtype, void* out, hdy_pack_desc* descs_host, int first_block);
int hdy_conv_pack_run(const hdy_pack_desc* descs_device, int ndesc, int total_blocks, void* stream);

/* y = act(scale[k] * conv(x, w)[.., k] + shift[k]) + res (+= y when accumulate).  scale/shift/res may be NULL (1 / 0 / none).
 * stats (optional, train-mode BN): [stat_slabs][2][K] floats, partial sums and sums of squares of the raw convolution (before
 * scale/shift/act); stat_slabs = what hdy_conv_stat_slabs(...) returned when the caller sized the array.  The launcher compares it with the
 * number of slabs the kernel it is about to start writes and returns HDY_EINVAL on a mismatch (a kernel-selection switch flipped
 * between the sizing query and the launch would otherwise write past the array or leave stale slabs for hdy_bn_finalize).  out_f32: write fp32 even when dtype is bf16 (detection logits).
 * stem: x is the hdy_stem_prep buffer; requires C=3, R=S=6, stride=2, pad=2, ldx=4. */
int hdy_conv_fwd(const void* x, int ldx, const void* w_packed, const float* scale, const float* shift, const void* res, int ldr, void* y,
                 int ldy, float* stats, int stat_slabs, int N, int H, int W, int C, int K, int R, int S, int stride, int pad, int act, int accumulate,
                 int dtype, int out_f32, int stem, void* stream);

/* dx[N][H][W][C] (+)= conv_transpose(dy[N][Ho][Wo][K], w); stride 1 or 2. */
int hdy_conv_dgrad(const void* dy, int lddy, const void* w_packed_dgrad, void* dx, int lddx, int N, int H, int W, int C, int K, int R,
                   int S, int stride, int pad, int accumulate, int dtype, void* stream);

/* grad_a[K_a][C][R][S] (and grad_b[K_b][..] = the following K_b output channels, for two convs fused along K)
 * (+)= dW, fp32, deterministic (slab reduction, no atomics). */
size_t hdy_conv_wgrad_workspace_bytes(int N, int H, int W, int C, int K, int R, int S, int stride, int pad, int dtype, int stem);
int hdy_conv_wgrad(const void* x, int ldx, const void* dy, int lddy, int N, int H, int W, int C, int K, int R, int S, int stride, int pad,
                   float* grad_a, int K_a, float* grad_b, int K_b, int accumulate, void* workspace, size_t ws_bytes, int dtype, int stem,
                   void* stream);

/* Fused backward of a 1x1 Conv + BatchNorm(train) + SiLU unit (metayolo/models/layers.py:31-38 under autograd, train.py:472): from
 * the output gradient dz ([0,Ka) from dz_a, [Ka,K) from dz_b), the raw conv output y, the BatchNorm coefficients and c1 / c2 of
 * hdy_bn_act_bwd(dy = NULL), computes dy = scale*(dz*silu'(u) - c1 - xhat*c2) on the fly and from it BOTH dx (+)= dy * W (NULL: skipped)
 * and the weight gradient grad_a / grad_b (+)= dy^T * x (NULL: skipped) in one pass: dy never goes to HBM.  bf16, C == K in {32, 64, 128}
 * (hdy_conv1x1_bwd_fused_ok); w_packed_dgrad = hdy_conv_pack(kind = HDY_PACK_DGRAD). */
/* Producer-side BatchNorm-backward statistics.  The kernel that writes the LAST contribution of a gradient tensor (a data-gradient
 * launch) can also serve the reduce pass of the Conv+BN+act unit(s) whose output gradient that tensor is: for its output channels
 * [c0, c1) it reads the unit's raw conv output y (same pixels; channel c0 <-> element 0 of y / scale / shift), forms
 * du = dz * act'(y*scale + shift) and writes per workgroup one fp32 slab [2][c1 - c0] = (SUM du, SUM du*y) to slabs[wg][2][c1-c0].
 * hdy_bn_bwd_finalize_slabs (SUM du*xhat = invstd * (SUM du*y - mean * SUM du)) then gives dgamma / dbeta / c1 / c2 without the
 * unit's own pass over dz and y.  Served by launches whose gradient is at most 64 channels wide (the wider instances have no
 * registers to spare): hdy_conv_dgrad_stat_slabs / hdy_conv1x1_bwd_fused_stat_slabs return 0 otherwise.
 * (reference: what autograd's BatchNorm backward reduces, metayolo/models/layers.py:37 under train.py:472) */
typedef struct {
    const void* y; int ldy;
    const float *scale, *shift;
    float* slabs;
    int c0, c1, act;
    int nslabs;          /* slabs the caller's array holds (the hdy_*_stat_slabs query it was sized with): HDY_EINVAL unless the launch writes exactly that many */
} hdy_stat_req;
int hdy_conv1x1_bwd_fused_stat_slabs(long long M, int C, int K, int dtype);
/* slabs a stats-serving launch writes (= its workgroups); 0: this shape cannot serve statistics */
int hdy_conv_dgrad_stat_slabs(int N, int H, int W, int C, int K, int R, int S, int stride, int pad, int dtype);
int hdy_conv_dgrad_stats(const void* dy, int lddy, const void* w_packed_dgrad, void* dx, int lddx, int N, int H, int W, int C, int K, int R,
                         int S, int stride, int pad, int accumulate, int dtype, const hdy_stat_req* stats, int nstat, void* stream);
int hdy_conv1x1_bwd_fused_stats(const void* dz_a, int lddz_a, const void* dz_b, int lddz_b, int Ka, const void* y, int ldy, const float* scale,
                                const float* shift, const float* mean, const float* invstd, const float* c1, const float* c2, const void* x, int ldx,
                                const void* w_packed_dgrad, void* dx, int lddx, int accumulate_dx, float* grad_a, int K_a, float* grad_b, int K_b,
                                int accumulate_w, long long M, int C, int K, void* workspace, size_t ws_bytes, int dtype, const hdy_stat_req* stats,
                                int nstat, void* stream);
/* from `nslabs` slabs [2][K] of (SUM du, SUM du*y): dbeta (+)= SUM du, dgamma (+)= invstd * (SUM du*y - mean * SUM du);
 * c1 = dbeta / count, c2 = dgamma / count (either may be NULL) */
int hdy_bn_bwd_finalize_slabs(const float* slabs, int nslabs, int K, long long count, const float* mean, const float* invstd, float* dgamma,
                              float* dbeta, int accumulate, float* c1, float* c2, void* stream);
/* the apply pass alone: dy = scale * (dz*act'(u) - c1 - xhat*c2) with c1 / c2 given */
int hdy_bn_act_bwd_apply(const void* dz, int lddz, const void* dz_b, int lddz_b, int Ka, const void* y, int ldy, const float* scale,
                         const float* shift, const float* mean, const float* invstd, const float* c1, const float* c2, void* dy, int lddy,
                         long long M, int K, int act, int dtype, void* stream);
int hdy_conv1x1_bwd_fused_ok(int C, int K, int dtype);
int hdy_conv1x1_bwd_fused_grid(long long M, int K);
size_t hdy_conv1x1_bwd_fused_workspace_bytes(long long M, int C, int K);
int hdy_conv1x1_bwd_fused(const void* dz_a, int lddz_a, const void* dz_b, int lddz_b, int Ka, const void* y, int ldy, const float* scale,
                          const float* shift, const float* mean, const float* invstd, const float* c1, const float* c2, const void* x, int ldx,
                          const void* w_packed_dgrad, void* dx, int lddx, int accumulate_dx, float* grad_a, int K_a, float* grad_b, int K_b,
                          int accumulate_w, long long M, int C, int K, void* workspace, size_t ws_bytes, int dtype, void* stream);

/* ---- BatchNorm + SiLU (+ residual) ---------------------------------------------------------------------------
 * Replaces nn.BatchNorm2d (eps 1e-3, momentum 0.03: metayolo/models/utils_torch.py:47-49) and nn.SiLU in
 * Conv.forward (metayolo/models/layers.py:37-38), the shortcut add of Bottleneck.forward (:97), their backward,
 * and the eval-time folding of fuse_conv_and_bn (metayolo/models/utils_torch.py:79-99). */
/* stats: [mtiles][2][stats_ld] slabs from hdy_conv_fwd (channel slice of K).  workspace (optional, enables the parallel
 * two-stage reduction for mtiles > 1024): ws_bytes >= hdy_bn_finalize_workspace_bytes(mtiles, K), 8-byte aligned (HDY_EINVAL when a
 * non-NULL workspace is smaller). */
size_t hdy_bn_finalize_workspace_bytes(int mtiles, int K);
int hdy_bn_finalize(const float* stats, int stats_ld, int mtiles, int K, long long count, const float* gamma, const float* beta, float* running_mean,
                    float* running_var, float eps, float momentum, float* scale, float* shift, float* save_mean, float* save_invstd,
                    void* workspace, size_t ws_bytes, void* stream);
int hdy_bn_eval_coeffs(const float* gamma, const float* beta, const float* running_mean, const float* running_var, float eps, int K,
                       float* scale, float* shift, void* stream);
/* The same for every BatchNorm of an inference plan in ONE launch: the caller fills the descriptors on the host, copies them into
 * device memory once and replays hdy_bn_eval_coeffs_batch before every forward (57 launches of 5 us otherwise for yolov5s). */
typedef struct hdy_bn_eval_desc {
    const float* gamma;
    const float* beta;
    const float* running_mean;
    const float* running_var;
    float* scale;
    float* shift;
    int K;
    float eps;
} hdy_bn_eval_desc;
int hdy_bn_eval_coeffs_batch(const hdy_bn_eval_desc* descs_device, int ndesc, void* stream);
int hdy_bn_act_fwd(const void* y, int ldy, const float* scale, const float* shift, const void* res, int ldr, void* z, int ldz,
                   long long M, int K, int act, int dtype, void* stream);
int hdy_bn_bwd_blocks(long long M);
/* workspace: ws_bytes >= hdy_bn_bwd_workspace_bytes(M, K) = (hdy_bn_bwd_blocks(M) * 2 * K + 2 * K) floats (HDY_EINVAL otherwise) */
size_t hdy_bn_bwd_workspace_bytes(long long M, int K);
/* mean == invstd == NULL: frozen statistics (FrozenBatchNorm2d, metayolo/models/utils_torch.py:180-203): dy = scale * dz * act'(u),
 * dgamma / dbeta untouched. */
int hdy_bn_act_bwd(const void* dz, int lddz, const void* y, int ldy, const float* scale, const float* shift, const float* mean,
                   const float* invstd, void* dy, int lddy, float* dgamma, float* dbeta, int accumulate, long long M, int K, int act,
                   int dtype, float* workspace, size_t ws_bytes, void* stream);
/* dy == NULL: statistics only (reduce + finalize: dgamma, dbeta, and c1 = dbeta/M, c2 = dgamma/M left in
 * workspace[hdy_bn_bwd_blocks(M)*2*K .. +2K)) for a consumer that applies them itself (hdy_conv1x1_bwd_fused). */
/* The same three passes for the PAIR of BatchNorms behind a C3's cv1 | cv2 (metayolo/models/layers.py:126-131: both read the same
 * input, so their convolutions run as one K = Ka + Kb wide launch): BatchNorm is per channel, so the pair is one K-wide layer; only
 * what the two modules own separately splits at Ka — parameters, running statistics and parameter gradients (finalize), the two
 * outputs (z_a: cv1's activation, z_b: cv2's slice of the concat buffer) and the two gradient sources (dz_a, dz_b).  One pass over
 * the 2c-wide raw tensor instead of two passes over half-width slices (K = 32 halves read 64 of every 128 bytes). */
int hdy_bn_finalize_pair(const float* stats, int stats_ld, int mtiles, int K, int Ka, long long count, const float* gamma_a, const float* beta_a,
                         float* running_mean_a, float* running_var_a, const float* gamma_b, const float* beta_b, float* running_mean_b,
                         float* running_var_b, float eps, float momentum, float* scale, float* shift, float* save_mean, float* save_invstd,
                         void* workspace, size_t ws_bytes, void* stream);
int hdy_bn_act_fwd_pair(const void* y, int ldy, const float* scale, const float* shift, void* z_a, int ldz_a, void* z_b, int ldz_b, int Ka,
                        long long M, int K, int act, int dtype, void* stream);
int hdy_bn_act_bwd_pair(const void* dz_a, int lddz_a, const void* dz_b, int lddz_b, int Ka, const void* y, int ldy, const float* scale,
                        const float* shift, const float* mean, const float* invstd, void* dy, int lddy, float* dgamma_a, float* dbeta_a,
                        float* dgamma_b, float* dbeta_b, int accumulate, long long M, int K, int act, int dtype, float* workspace, size_t ws_bytes, void* stream);
int hdy_add_inplace(void* out, int ldo, const void* a, int lda, long long M, int K, int dtype, void* stream);
/* out[k] (+)= sum_m dz[m][k]: bias gradient of Detect's conv (yolo_head.py:112).  workspace: ws_bytes >= hdy_colsum_workspace_bytes(M, K) = hdy_bn_bwd_blocks(M)*2*K floats */
size_t hdy_colsum_workspace_bytes(long long M, int K);
int hdy_colsum(const void* dz, int lddz, long long M, int K, float* out, int accumulate, int dtype, float* workspace, size_t ws_bytes, void* stream);

/* ---- SPPF pooling, upsample, layout --------------------------------------------------------------------------
 * Replaces nn.MaxPool2d(5,1,2) x3 of SPPF.forward (metayolo/models/layers.py:181-189), nn.Upsample(None,2,'nearest')
 * (hub yaml fpn rows) and the NCHW image hand-off (train.py:432, val_nuclei.py:135). */
int hdy_sppf_pool_fwd(const void* x, void* y1, void* y2, void* y3, int ld, unsigned char* idx1, unsigned char* idx2, unsigned char* idx3,
                      int N, int H, int W, int C, int dtype, void* stream);
int hdy_sppf_pool_bwd(const void* g0, const void* g1, const void* g2, const void* g3, int ldg, const unsigned char* idx1,
                      const unsigned char* idx2, const unsigned char* idx3, void* dx, int lddx, int N, int H, int W, int C, int dtype,
                      void* stream);
int hdy_upsample2x_fwd(const void* x, int ldx, void* y, int ldy, int N, int H, int W, int C, int dtype, void* stream);
int hdy_upsample2x_bwd(const void* dy, int lddy, void* dx, int lddx, int N, int H, int W, int C, int accumulate, int dtype, void* stream);
int hdy_stem_prep(const float* img_nchw, void* out, int B, int H, int W, int pad, int dtype, void* stream);
int hdy_nchw_to_nhwc(const float* src, void* dst, int ldd, int N, int C, int H, int W, int dtype, void* stream);

/* ---- detection head ------------------------------------------------------------------------------------------
 * hdy_decode replaces Detect.compute_proposals and the level-id pad + cat of compute_outputs
 * (metayolo/models/yolo_head.py:185-213, :311-312, :419-429): logits (b,a,y,x,o) addressed through element strides
 * (sb,sa,sy,sx; o contiguous) -> out[b][row_offset + (a*ny + y)*nx + x][0..no] = cx,cy,w,h (pixels), sigmoid(obj),
 * sigmoid(cls..), level id.  anchor_px: na*2 HOST floats (anchor w,h in pixels).
 *
 * hdy_nms_batched replaces nms_per_image (metayolo/models/utils_general.py:299-356; class_aware=0, the path's
 * default: class-agnostic, ranked by objectness, boxes with w or h < min_wh dropped, obj > conf strict) and
 * non_max_suppression (:423-523; class_aware=1) including torchvision.ops.nms / remove_small_boxes.
 * preds [B][N][row] fp32 with row = 5 + nc + extra.  Outputs per tile: keep[max_det] original row indices in
 * descending-score order (stable: ties by lower row), -1 padded; n_keep; and the gathered rows.
 * max_det: any positive value, as the reference's `[:max_det]` slice (utils_general.py:342); up to 4096 the kept list lives in LDS, beyond
 * that in the workspace (round 6).  workspace (16-byte aligned): hdy_nms_workspace_bytes_for(B, N, max_det) (= hdy_nms_workspace_bytes(B, N)
 * for max_det <= 4096). */
int hdy_decode(const float* det, long long sb, long long sa, long long sy, long long sx, const float* anchor_px, float stride, float* out,
               int row_offset, int rows_per_image, int level_id, int B, int na, int ny, int nx, int no, void* stream);
/* autograd's logits gradient (b,a,y,x,o; element strides) -> NHWC [B][ny][nx][ldo] of dtype, channel a*no+o, zero padded */
int hdy_det_grad_pack(const float* g, long long sb, long long sa, long long sy, long long sx, long long so, void* out, int ldo, int B, int na,
                      int ny, int nx, int no, int dtype, void* stream);
size_t hdy_nms_workspace_bytes(int B, int N);
size_t hdy_nms_workspace_bytes_for(int B, int N, int max_det);
int hdy_nms_batched(const float* preds, int B, int N, int row, int nc, float conf, float iou, int max_det, float min_wh, int class_aware,
                    long long* keep, int* n_keep, float* out_boxes, float* out_scores, float* out_extra, float* out_conf, int* out_cls,
                    void* workspace, size_t ws_bytes, void* stream);

/* Tail of Detect.compute_outputs (metayolo/models/yolo_head.py:335-345) on hdy_nms_batched's padded rows, whole batch, one launch:
 * hierarchical scores in place on scores [B][max_det][1 + nc] (pairs: npairs x (child, parent) column indices in the order the reference
 * applies them: child *= parent), then per kept box score / label (best class if > conf, else objectness / -100; multi_label: all 1 + nc
 * scores and score > conf flags).  Outputs are COMPACTED: image b's rows start at n_keep[0] + .. + n_keep[b - 1].  out_boxes [T][4],
 * out_scores [T] (multi_label: [T][1 + nc]), out_labels int64 [T] (multi_label: uint8 [T][1 + nc]) with T >= the total; offsets [B + 1]
 * (optional) receives the row offsets. */
int hdy_det_outputs(float* scores, const float* boxes, const int* n_keep, int B, int max_det, int nc, const int* pairs, int npairs, float conf,
                    int multi_label, float* out_boxes, float* out_scores, void* out_labels, int* offsets, void* stream);

/* torchvision.ops.nms on explicit boxes, as the reference calls it outside nms_per_image (Ensemble.merge, metayolo/models/yolo.py:189-199):
 * boxes_scores [B][N][5] = (x1, y1, x2, y2, score >= 0) fp32; every row is a candidate; keep[B][max_det] row indices in descending
 * score order (stable), -1 padded; n_keep[B].  Same kernel and workspace rule as hdy_nms_batched (any max_det). */
int hdy_nms_boxes(const float* boxes_scores, int B, int N, float iou, int max_det, long long* keep, int* n_keep, void* workspace,
                  size_t ws_bytes, void* stream);

/* The same result as hdy_nms_boxes with B = 1 (same kept rows, same order, bit for bit) for ONE large set of explicit boxes, computed by
 * the whole chip instead of one workgroup: the merge of a whole slide's tiles (evaluation.py inference_on_slide -> Detect.merge_outputs ->
 * utils_general.nms), Ensemble.merge (metayolo/models/yolo.py:189-199) and the torchvision.ops.nms calls of utils_general.py's
 * non_max_suppression option branches.  Pipeline (csrc/nms_grid.hip): 64-bit rank keys, multi-workgroup bitonic sort, a hierarchy of uniform
 * grids over the box centres (one level per octave of box size; one table for all levels, hashed when the cells outnumber its entries),
 * then rounds over an undecided / kept / suppressed state per box, one launch per round, until no box is undecided; kept flags are
 * compacted in rank order.
 * Split in three so that NO piece synchronises (all three can be listed for hdy_exec_run); the caller owns the loop:
 *   hdy_nms_grid_begin   keys, sort, cell index.  boxes_scores [M][5] = (x1, y1, x2, y2, score) fp32.
 *   hdy_nms_grid_round   n_rounds launches, numbered first_round, first_round + 1, ...: the caller continues the numbering in the next call.
 *                        A round that finds nothing undecided does nothing.  iou in [0, 1].
 *   hdy_nms_grid_finish  keep[max_det] (row indices in descending score order, ties by lower row, -1 padded), n_keep[1], and
 *                        status[3] = {boxes still undecided, non-finite flag, rounds that had work (may vary by one or two between runs: a box may see a
 *                        neighbour's decision of the same launch; the result cannot)}.  The result is valid when status[0] == 0
 *                        and status[1] == 0; with status[0] > 0 run more rounds and finish again (finish may be repeated).  status[1] != 0:
 *                        a coordinate or a side length is not finite, the index cannot serve the set, use hdy_nms_boxes.
 * workspace (16-byte aligned): hdy_nms_grid_workspace_bytes(M), a function of M alone; the same buffer, untouched in between, for the
 * three calls.  1 <= M <= HDY_NMS_GRID_MAX_M.  Cost: a box visits the cells its extent covers on every occupied level, so the work follows the
 * number of overlapping pairs; a box that would visit more cells than there are higher-ranked boxes scans those instead (O(M) for that box
 * per round).  A chain of n boxes each suppressing the next takes n rounds.  All boxes piled on one spot is the quadratic worst case, as
 * for any NMS.  Results do not depend on the order in which atomics arrive: same input, same bits. */
#define HDY_NMS_GRID_MAX_M (1 << 24)
size_t hdy_nms_grid_workspace_bytes(int M);
int hdy_nms_grid_begin(const float* boxes_scores, int M, void* workspace, size_t ws_bytes, void* stream);
int hdy_nms_grid_round(int M, float iou, int first_round, int n_rounds, void* workspace, size_t ws_bytes, void* stream);
int hdy_nms_grid_finish(int M, int max_det, long long* keep, int* n_keep, int* status, void* workspace, size_t ws_bytes, void* stream);

/* ---- whole-slide inference from an 8-bit slide (csrc/slide.hip) ----------------------------------------------------------------
 * The slide stays as slide readers deliver it: 8-bit pixels [H][pitch_bytes] on the device, pixel_bytes = 3 (RGB) or 4 (RGBA, alpha ignored),
 * an explicit row pitch in BYTES (>= W * pixel_bytes: a cropped view of a larger slide needs no copy), addressed in 64 bits.  Tiles are named
 * by a device table origins int32 [n_origins][2] = (x0, y0) of their top-left corners, uploaded once per slide; the kernels are memory-safe
 * for any table content (a window or a part of it outside the slide reads as zero / counts nothing).
 *
 * hdy_slide_tiles_u8 replaces the reference's per-ROI crop + `/ 255` normalisation + NCHW batch in front of the model call (the ROI protocol
 * around Detect.merge_outputs, metayolo/models/yolo_head.py:450-462; images are normalised with `/ 255` in val_nuclei.py:137) and this
 * library's own hdy_stem_prep / hdy_nchw_to_nhwc behind it: tiles [first, first + count) of the table go straight into the buffer the first
 * convolution reads.  ldd == 0: the hdy_stem_prep layout [count][th + 2 pad][tw + 2 pad][4] (zero frame, zero 4th channel), out 16-byte
 * aligned; ldd >= 3 (pad must be 0): pitched NHWC [count][th][tw][ldd], channels 0..2 written, as hdy_nchw_to_nhwc writes a 3-channel image.
 * Pixel value: float(v) / 255 correctly rounded to fp32 (a 256-entry table made on the host with IEEE division; NOT v * (1 / 255)), then
 * converted to dtype as every other kernel converts.  out_elems = elements of dtype `out` holds: HDY_EINVAL unless it is exactly what the call
 * writes.  Source bytes are read as whole aligned dwords: up to 3 bytes beside a row's pixels (never outside their page) may be read.
 *
 * hdy_slide_append replaces Detect.merge_outputs (yolo_head.py:450-462: per ROI `boxes + (x0, y0, x0, y0)`, then cat): the batch's compacted
 * detections (hdy_det_outputs, single label: boxes [in_rows][4], scores [in_rows], labels int64 [in_rows], tile b's rows at
 * n_keep[0] + .. + n_keep[b - 1]; B <= 1024 tiles = rows [first, first + B) of the table) are appended to slide-wide arrays of `capacity` rows at
 * cursor[0], each box shifted by its tile's origin with one fp32 add per coordinate, in tile order then row order; cursor[0] moves by the rows
 * written.  cursor int32 [2] lives on the device (zeroed by the caller before the first batch): rows that would pass `capacity` (or lie beyond
 * in_rows) are dropped and cursor[1] is set to 1 — nothing is written past the end.  One workgroup, no atomics: repeats are bit-identical, and a
 * slide needs no device-to-host copy per batch.
 *
 * hdy_slide_tissue_u8 (no reference counterpart: the reference has no blank-tile rule): counts[t] = pixels of tile t's th x tw window, clipped
 * to the slide, that are NOT background, a pixel being background when min(R, G, B) >= background.  Exact integer counts, one workgroup per
 * tile; n_counts must equal n_origins. */
int hdy_slide_tiles_u8(const unsigned char* slide, long long pitch_bytes, int pixel_bytes, int H, int W, const int* origins, int n_origins,
                       int first, int count, void* out, long long out_elems, int th, int tw, int pad, int ldd, int dtype, void* stream);
int hdy_slide_append(const float* boxes, const float* scores, const long long* labels, const int* n_keep, int B, int in_rows, const int* origins,
                     int n_origins, int first, float* out_boxes, float* out_scores, long long* out_labels, int capacity, int* cursor, void* stream);
int hdy_slide_tissue_u8(const unsigned char* slide, long long pitch_bytes, int pixel_bytes, int H, int W, const int* origins, int n_origins, int th,
                        int tw, int background, int* counts, int n_counts, void* stream);

/* ---- training augmentation from an 8-bit tile bank (csrc/augment.hip) ---------------------------------------------------------------
 * Replaces the training branch of the reference's loader (metayolo/datasets.py TorchDataset.__getitem__ on the keep_res <= 0 path, detection
 * annotations without masks): per output image a k x k mosaic of cells, each cell one source tile through train_proc (random_hsv ->
 * random_projective into a patch x patch canvas with border value cval -> random_flip: hflip, vflip, transpose), then a random img_size crop,
 * the crop's and the final remove_invalid_objects, and target_to_tensors' normalisation.  The parameters are drawn and the matrices composed
 * on the host in float64 (hd_yolo_amd/augment.py); the two kernels apply them.  The pixel arithmetic is this library's own (the reference
 * calls cv2 and pins no version) and is stated here in full, so that tests/augment_ref.py reproduces both kernels bit for bit.
 *
 * Bank: n tiles of H x W 8-bit pixels, tile t's row y at bank + t * tile_stride_bytes + y * pitch_bytes, pixel_bytes = 3 (RGB) or 4 (RGBA,
 * alpha ignored); a cropped view of a larger bank needs no copy.  Boxes of the bank: bank_boxes fp32 [M][4] xyxy in source pixels (16-byte
 * aligned), bank_labels int64 [M], offsets int64 [n + 1] (tile t owns rows [offsets[t], offsets[t + 1])).
 *
 * Cell table: B * k * k records of HDY_AUG_CELL_BYTES, image-major, then cell row r, then cell column c.  A record is 24 little-endian words
 *   [0] source tile (int32)   [1..9] inverse matrix Mi (canvas -> source, fp32 row-major)   [10] flags: 1 hflip, 2 vflip, 4 transpose, 8 HSV,
 *   16 perspective divide   [11..19] forward matrix M (source -> canvas)   [20] scale   [21..23] zero
 * followed by three 256-byte tables (hue, saturation, value).  crop: int32 [B][2] = (x, y) of the crop window in the mosaic.  Both kernels are
 * memory-safe for any table content: a source index outside [0, n) reads as cval and owns no boxes; a crop offset outside
 * [0, k * patch - img_size] gives an image of cval and no boxes; offsets rows that are negative, decreasing or beyond M own no boxes.
 *
 * hdy_augment_tiles_u8 writes out (B, 3, img_size, img_size) NCHW of dtype; out_elems must be exactly that many elements (else HDY_EINVAL);
 * out 16-byte aligned; k <= 8; 4 <= patch <= 32768; img_size <= k * patch.  Output pixel (ox, oy) of image b:
 *   X = ox + crop_x, Y = oy + crop_y;  c = X / patch, r = Y / patch (cell);  u = X - c patch, v = Y - r patch
 *   transpose: swap(u, v);  vflip: v = patch - 1 - v;  hflip: u = patch - 1 - u          (the three flips undone, last one first)
 *   sx = (Mi0 u + Mi1 v) + Mi2, sy = (Mi3 u + Mi4 v) + Mi5 in fp32, every product and sum rounded on its own (no FMA); with the perspective
 *   flag sw = (Mi6 u + Mi7 v) + Mi8, sx = sx / sw, sy = sy / sw
 *   qx = rint(32 sx), qy = rint(32 sy) (ties to even; 1/32 pixel, the convention of 8-bit warpAffine); |32 s| > 2^24 or NaN: the pixel is cval
 *   x0 = qx >> 5, fx = qx & 31, y0 = qy >> 5, fy = qy & 31;  texels t00 = (x0, y0), t01 = (x0 + 1, y0), t10 = (x0, y0 + 1), t11: a position
 *   outside the tile reads (cval, cval, cval); one inside goes through the HSV round trip when the flag is set (before interpolation)
 *   per channel  p = (t00 (32 - fx)(32 - fy) + t01 fx (32 - fy) + t10 (32 - fx) fy + t11 fx fy + 512) >> 10
 *   out = table[p], the correctly rounded p / 255 of hdy_slide_tiles_u8, converted to dtype.
 * HSV round trip of a pixel (r, g, b), all integers, `/` truncating on non-negative operands:
 *   V = max, d = V - min, S = V ? (255 d + (V >> 1)) / V : 0
 *   H = 0 when d == 0, else off + (60 (num + d) + d) / (2 d) - 30 with (num, off) = (g - b, 0) if V == r, else (b - r, 60) if V == g, else
 *   (r - g, 120); H += 180 when negative                                                   (H in 0 .. 179)
 *   H' = hue[H] (minus 180 when >= 180), S' = sat[S], V' = val[V];  sec = H' / 30, f = H' - 30 sec
 *   p = (V' (255 - S') + 127) / 255,  q = (V' (7650 - S' f) + 3825) / 7650,  t = (V' (7650 - S' (30 - f)) + 3825) / 7650
 *   (r, g, b) = (V', t, p), (q, V', p), (p, V', t), (p, q, V'), (t, p, V'), (V', p, q) for sec = 0 .. 5.
 * Source bytes are read as whole aligned dwords: up to 3 bytes beside a pixel (never outside its page) may be read.
 *
 * hdy_augment_boxes ("Targets") writes the kept boxes of the batch compactly: out_boxes fp32 [cap][4] (xyxy / img_size, 16-byte aligned),
 * out_labels int64 [cap], out_img fp32 [cap] (image index: the form hdy_det_targets takes), counts int32 [n_counts = B] rows per image, and
 * overflow[0] = 1 when more than cap rows were kept (else 0): the first cap rows are written, nothing beyond.  Order: image, then cell in
 * (r, c) order, then source order.  One workgroup, prefix sums, no atomics: repeats are bit-identical.  B * k * k <= 4096; of a tile's boxes
 * the first 65536 are read.  Per source box (x1, y1, x2, y2) of cell (r, c), fp32, every operation rounded on its own, in this order:
 *   corners (x1, y1), (x1, y2), (x2, y2), (x2, y1):  X = (x M0 + y M1) + M2, Y = (x M3 + y M4) + M5; with the perspective flag
 *   Wd = (x M6 + y M7) + M8, X = X / Wd, Y = Y / Wd;  X = min(max(X, 0), patch), Y alike                       (warp_coords, Mask(clip=True))
 *   box = (min X, min Y, max X, max Y), or zeros when all four X are zero                                       (Mask.box)
 *   w1 = x2 scale - x1 scale, h1 alike; w2, h2 of box; kept when w2 > 2, h2 > 2, (w2 h2) / (w1 h1 + 1e-16) > 0.1 and
 *   max(w2 / (h2 + 1e-16), h2 / (w2 + 1e-16)) < 100                                                             (box_candidates)
 *   hflip: (|x2 - patch|, |y1|, |x1 - patch|, |y2|);  vflip: (|x1|, |y2 - patch|, |x2|, |y1 - patch|);  transpose: (y1, x1, y2, x2)
 *   x += (c patch - crop_x), y += (r patch - crop_y)      (the integer difference is exact in fp32)             (pad_annotation, crop_annotation)
 *   dropped unless x1 < x2 and y1 < y2 (remove_invalid_objects after the crop evaluates its filter on the UNCLIPPED box: it removes nothing)
 *   clipped to [0, img_size]; dropped unless x1 < x2 - 10 and y1 < y2 - 10                                      (the final filter)
 *   out = box / img_size. */
#define HDY_AUG_CELL_BYTES 864
int hdy_augment_tiles_u8(const unsigned char* bank, long long tile_stride_bytes, long long pitch_bytes, int pixel_bytes, int n, int H, int W,
                         const void* cells, int n_cells, const int* crop, int B, int patch, int k, int img_size, int cval, void* out,
                         long long out_elems, int dtype, void* stream);
int hdy_augment_boxes(const float* bank_boxes, const long long* bank_labels, const long long* offsets, int n, int M, const void* cells, int n_cells,
                      const int* crop, int B, int patch, int k, int img_size, float* out_boxes, long long* out_labels, float* out_img, int cap,
                      int* counts, int n_counts, int* overflow, void* stream);

/* ---- instance masks through the device augmentation (csrc/augment_masks.hip) ----------------------------------------------------------
 * Replaces what the reference's loader does to the masks of detection annotations (metayolo/datasets.py random_projective :329-337, the flips,
 * the mosaic, the crop, target_to_tensors :482-494).  The reference warps polygons and resizes with cv2 (absent here, unpinned upstream), so
 * the arithmetic is this library's own, stated here in full; tests/augment_mask_ref.py restates it over the whole canvas, bit for bit.  The
 * reference's rules are kept: a masked object's box is the box of its warped mask, its candidate test takes 0.01 for 0.1, its target is the
 * mask cropped to the (integer) box and resized bilinearly to 28 x 28, a mask of fewer than 25 pixels gives a zero target, an object without
 * a mask keeps the corner box, the 0.1 test and a zero target.
 *
 * Instance map: instances uint16 [n][H][W], dense, beside the bank of hdy_augment_tiles_u8 (same n, H, W).  A pixel holds the index w of its
 * owner among its tile's boxes (bank row offsets[t] + w) or 0xFFFF (background): one owner per pixel.  has_mask uint8 [M]: 1 for a bank row
 * that owns at least one pixel.  Every pixel (px, py) of an object must lie in its box grown to pixel edges, floor(x1) <= px < ceil(x2) and
 * alike in y (hd_yolo_amd.augment.TileBank validates it): hdy_augment_mask_extents scans only a canvas region derived from that box.  Cell
 * table, crop, B, patch, k, img_size: those of the two calls above, and the same limits.  All three entry points are memory-safe for any table
 * content (a source index outside [0, n), a crop offset out of range, offsets rows negative / decreasing / beyond M own nothing and read
 * nothing; instance-map reads are bounds-checked like texel reads) and deterministic (no atomics, fixed reduction order).
 *
 * Membership: canvas pixel (u, v), integers in [0, patch)^2 in pre-flip canvas coordinates, belongs to the warped mask of object w of cell ci
 * when, with sx, sy (and sw with the perspective flag) computed from Mi exactly as hdy_augment_tiles_u8 computes them,
 *   qx = rint(32 sx), qy = rint(32 sy)  (|32 s| > 2^24 or NaN: not a member);  xn = (qx + 16) >> 5, yn = (qy + 16) >> 5 (nearest source pixel)
 *   0 <= xn < W, 0 <= yn < H, the cell's source tile src is in [0, n), w < 0xFFFF and instances[src][yn][xn] == w.
 * Image-space mask of (ci, w) at image pixel (ox, oy) of image b: X = ox + crop_x, Y = oy + crop_y; zero unless X / patch == c and Y / patch
 * == r (the object's cell); else the membership of (u, v) = (X - c patch, Y - r patch) after transpose: swap(u, v); vflip: v = patch - 1 - v;
 * hflip: u = patch - 1 - u (as the image kernel undoes them).  The image position of canvas pixel (u, v) is the inverse, all integers:
 *   hflip: u = patch - 1 - u;  vflip: v = patch - 1 - v;  transpose: swap(u, v);  ox = u + c patch - crop_x, oy = v + r patch - crop_y.
 *
 * hdy_augment_mask_extents: a candidate is (cell ci, object w) with w < the box count of the cell's source tile (as hdy_augment_boxes counts
 * it), w < pitch.  For every candidate one record of 8 int32 is written to ws[(ci * pitch + w) * 8 ..] (ws 16-byte aligned; ws_bytes >=
 * n_cells * pitch * 32 else HDY_EINVAL; 1 <= pitch <= 65535, at least the bank's largest box count per tile):
 *   [0] count: members over ALL canvas pixels of the cell   [1] umin [2] umax [3] vmin [4] vmax of the members (0 when count == 0)
 *   [5] area_img: members whose image position lies in [0, img_size)^2   [6] [7] zero
 * A candidate without has_mask (or with w = 0xFFFF) gets the all-zero record; entries that are no candidate are not written.  The kernel may
 * scan less than the canvas — the forward-warped box grown to pixel edges, plus a margin — but the definition is the whole canvas.
 *
 * hdy_augment_boxes_masks: hdy_augment_boxes with, for a row with has_mask (and w < pitch), the canvas box (umin, vmin, umax + 1, vmax + 1) as
 * floats from its record, or the zero box when count == 0, in place of the corner box, and 0.01 in place of 0.1 in the candidate test (w1, h1
 * stay those of the source box).  Everything else — order, flips, offsets, the crop's filter, the clip, x1 < x2 - 10, / img_size, cap,
 * overflow, counts, the 4096-cell limit — is that entry point's text; a row without a mask goes through it unchanged.  Additional outputs:
 * out_ref int32 [cap][2] = (ci, w) per written row, total[0] = rows written = min(kept, cap).
 *
 * hdy_augment_mask_targets: out_masks fp32 [cap][28][28] (out_elems == cap * 784 else HDY_EINVAL; 16-byte aligned).  One workgroup per row; a
 * row >= total[0] (read on the device: no host synchronisation) is not written.  A written row is zero when it has no mask, when area_img <
 * 25, or when its pixel box has w < 1 or h < 1, the pixel box being x1 = rint(out_boxes x1 * img_size) and alike, clamped to [0, img_size],
 * w = x2 - x1, h = y2 - y1 (a masked row's pixel box is integer: the division and the product move it by less than 1/16).  Otherwise, for
 * destination (i, j), fp32, every operation rounded on its own:
 *   fx = (j + 0.5) * (w / 28) - 0.5;  x0 = floor(fx), a = fx - x0;  x0 < 0: x0 = 0, a = 0;  x0 >= w - 1: x0 = w - 1, a = 0;  xb = min(x0 + 1, w - 1)
 *   the same in y with fy, y0, b, yb (the half-pixel convention of cv2.INTER_LINEAR);  taps m00 = mask(x1 + x0, y1 + y0), m01 = mask(x1 + xb,
 *   y1 + y0), m10 = mask(x1 + x0, y1 + yb), m11 = mask(x1 + xb, y1 + yb) of the image-space mask (0 or 1)
 *   out = (m00 (1 - a) + m01 a) (1 - b) + (m10 (1 - a) + m11 a) b.
 * Not implemented: polygon or RLE input, mask_order other than bilinear, keep_res > 0. */
int hdy_augment_mask_extents(const uint16_t* instances, int n, int H, int W, const float* bank_boxes, const unsigned char* has_mask,
                             const long long* offsets, int M, const void* cells, int n_cells, const int* crop, int B, int patch, int k, int img_size,
                             void* ws, long long ws_bytes, int pitch, void* stream);
int hdy_augment_boxes_masks(const float* bank_boxes, const long long* bank_labels, const unsigned char* has_mask, const long long* offsets, int n,
                            int M, const void* cells, int n_cells, const int* crop, int B, int patch, int k, int img_size, const void* ws,
                            long long ws_bytes, int pitch, float* out_boxes, long long* out_labels, float* out_img, int* out_ref, int cap,
                            int* counts, int n_counts, int* overflow, int* total, void* stream);
int hdy_augment_mask_targets(const uint16_t* instances, int n, int H, int W, const unsigned char* has_mask, const long long* offsets, int M,
                             const void* cells, int n_cells, const int* crop, int B, int patch, int k, int img_size, const void* ws,
                             long long ws_bytes, int pitch, const float* out_boxes, const int* out_ref, const int* total, int cap, float* out_masks,
                             long long out_elems, void* stream);

/* ---- detection scoring: AP matching for ragged batches and whole slides (csrc/score.hip) --------------------------------------------
 * Replaces the per-image work of APMeter.add and the matching half of APMeter.ap_per_class (metayolo/models/metrics.py:251-375: five
 * device-to-host copies, a CPU sort, a dense box_iou matrix, np.nonzero, an argsort over the pairs, two np.unique passes).  B images; image i
 * owns prediction rows [pred_off[i], pred_off[i + 1]) and truth rows [true_off[i], true_off[i + 1]) of the concatenated arrays (offsets int32
 * [B + 1] ON THE DEVICE, so a caller needs no read to launch; they are clamped into [0, capacity] on the device: any content is memory-safe;
 * rows outside every span are neither read nor written).  pred_boxes / true_boxes fp32 [capacity][4] xyxy, 16-byte aligned; pred_scores fp32;
 * labels int64.  Per image:
 *   1. IoU exactly as utils_general.box_iou on CPU fp32 (inter = max(min(x2, X2) - max(x1, X1), 0) * max(min(y2, Y2) - max(y1, Y1), 0),
 *      iou = inter / ((a + A) - inter), every operation rounded on its own).  A pair with IoU < pair_iou, or a NaN IoU, is no pair; a pair
 *      whose prediction or truth label is in `ignore` only marks the prediction as touched;
 *   2. otherwise the prediction keeps the truth of highest IoU (tie: lowest truth row);
 *   3. every truth is claimed by the prediction of highest score among those that kept it (tie: lower prediction row);
 *   4. a prediction is matched iff it won its claim and the two labels agree: hit[p] bit j = (its IoU >= iouv[j]), match[p] = the truth's row in
 *      the concatenated truth array, match_iou[p] = its IoU; unmatched: 0, -1, 0;
 *   5. live[p] = 0 iff the prediction was touched and is not matched (such predictions leave the precision / recall curves), else 1.
 * "row" in the two tie rules is the position in the concatenated arrays, or pred_row[p] / true_row[t] (int32, non-negative, distinct inside an
 * image; may be NULL) when given: a caller may then permute its inputs without changing any result.
 * iouv (n_iou in [1, 16] thresholds), pair_iou in (0, 1] and ignore (n_ignore in [0, 4] labels) are HOST values, read before the call returns.
 * Truths are walked in chunks of HDY_AP_TRUE_CHUNK by workgroups of HDY_AP_PRED_BLOCK predictions; a workgroup skips every chunk whose bounding
 * box does not overlap its own predictions' box (boxes with a non-finite coordinate are in neither box and always visited), which cannot change
 * a result.  workspace (16-byte aligned, hdy_ap_match_workspace_bytes, 0 = counts out of range; travels with its size): after the call its
 * first two uint64 hold the chunk pairs visited and the chunk pairs in total.  No allocation, no synchronisation, everything on `stream`; the
 * outputs are a pure function of the inputs (no dependence on atomic arrival order, HDY_AP_CHUNK or HDY_AP_NO_PRUNE).  All argument checks are made
 * before any launch. */
#define HDY_AP_PRED_BLOCK 256
#define HDY_AP_TRUE_CHUNK 256
#define HDY_AP_MAX_ROWS (1 << 28)
size_t hdy_ap_match_workspace_bytes(int n_img, int pred_capacity, int true_capacity);
int hdy_ap_match(const float* pred_boxes, const float* pred_scores, const long long* pred_labels, const int* pred_off, const int* pred_row,
                 int pred_capacity, const float* true_boxes, const long long* true_labels, const int* true_off, const int* true_row,
                 int true_capacity, int n_img, const float* iouv, int n_iou, float pair_iou, const long long* ignore, int n_ignore,
                 unsigned short* hit, unsigned char* live, int* match, float* match_iou, void* workspace, size_t ws_bytes, void* stream);

/* ---- mask paste: image-space instance masks, a slide label map and its areas (csrc/paste.hip) ------------------------------------------
 * hdy_paste_masks replaces torchvision.models.detection.roi_heads.paste_masks_in_image as the reference calls it (val_nuclei.py:31,169-176 on
 * every validation image, data.py:16,491); hdy_paste_label_map and hdy_label_areas give the whole-slide form the reference composes on the host
 * from those pasted masks (one nucleus segmentation of the slide instead of one canvas per nucleus).  The arithmetic is torchvision's published
 * algorithm (expand_boxes, paste_mask_in_image) with torch's CPU bilinear resize, stated here in full so that tests/paste_ref.py reproduces
 * both modes bit for bit.  Everything is fp32 and every product, sum and quotient is rounded on its own (no FMA).
 *
 * masks fp32 [R][M][M] (Detect.attach_masks' probabilities in box coordinates; HDY_PASTE_MIN_M <= M <= HDY_PASTE_MAX_M), boxes fp32 [R][4]
 * xyxy in canvas pixels, padding 0 or 1 (torchvision: 1).  Per row r:
 *   P = M + 2 padding; the mask is framed by `padding` rows and columns of zeros: patch[P][P]
 *   scale = float(P) / float(M)                                                                                   (expand_boxes)
 *   hx = ((x2 - x1) * 0.5f) * scale, cx = (x2 + x1) * 0.5f;  ex1 = cx - hx, ex2 = cx + hx;  y alike
 *   bx1 = int(ex1), bx2 = int(ex2), by1, by2: truncation toward zero (.to(int64)), not floor
 *   a row with a non-finite expanded coordinate, or one of magnitude >= 2^30, pastes nothing
 *   w = max(bx2 - bx1 + 1, 1), h = max(by2 - by1 + 1, 1): a degenerate box (x2 < x1) pastes one column
 *   the patch is resized to h x w (F.interpolate, bilinear, align_corners=False); along x, for destination column d in [0, w):
 *     sc = float(P) / float(w) (one IEEE division);  s = max(sc * (float(d) + 0.5f) - 0.5f, 0)
 *     i0 = int(s), i1 = i0 + (i0 < P - 1), l1 = s - float(i0), l0 = 1 - l1;  along y alike with h
 *   value(dy, dx) = ly0 * (lx0 * patch[iy0][ix0] + lx1 * patch[iy0][ix1]) + ly1 * (lx0 * patch[iy1][ix0] + lx1 * patch[iy1][ix1])
 *   it belongs to canvas pixel (bx1 + dx, by1 + dy); the resized patch covers [bx1, bx1 + w) x [by1, by1 + h), clipped to the output.
 * Rows whose mask label is negative arrive as all-zero masks (attach_masks) and therefore paste zeros / own nothing.
 *
 * hdy_paste_masks (dense mode): out fp32 [R][H][W], out_elems = R * H * W exactly (else HDY_EINVAL): the value where row r's box covers the
 * canvas, zero elsewhere; every element is written.  No atomics.
 * hdy_paste_label_map: map int32 [h][w] (map_elems = h * w exactly, 64-bit: it may pass 2^31) of the canvas window [x0, x0 + w) x [y0, y0 + h):
 * -1 = background, otherwise the lowest row r whose value at the pixel is >= threshold (after the slide NMS the rows are in descending score
 * order: the highest score owns the pixel).  The entry point fills the map with 0xFF bytes and one launch for all R rows does an unsigned
 * 32-bit atomic minimum per covered pixel: order-independent, so repeats are bit-identical.  R is a host value; no device-to-host copy.
 * hdy_label_areas: areas int32 [R], zeroed by the call; areas[r] = number of map entries equal to r (entries outside [0, R) are not counted).
 * Integer adds of run lengths: exact and order-independent.
 * HDY_EINVAL with a message: null pointers, M or padding out of range, sides outside [1, HDY_PASTE_MAX_SIDE], out_elems / map_elems that
 * differ from what the call writes.  All argument checks are made before any launch. */
#define HDY_PASTE_MIN_M 2
#define HDY_PASTE_MAX_M 62
#define HDY_PASTE_MAX_SIDE (1 << 29)
int hdy_paste_masks(const float* masks, int R, int M, int padding, const float* boxes, float* out, long long out_elems, int H, int W,
                    void* stream);
int hdy_paste_label_map(const float* masks, int R, int M, int padding, const float* boxes, float threshold, int x0, int y0, int* map,
                        long long map_elems, int h, int w, void* stream);
int hdy_label_areas(const int* map, long long map_elems, int* areas, int R, void* stream);

/* ---- mask scoring: label-map overlap and the AP matching on mask IoU (csrc/mask_score.hip) ----------------------------------------------
 * Replaces get_mask_ious (utils_nucls.py:480-489: a dense (n_true, n_pred, H * W) product of 0 / 1 float masks) and the mask branch of
 * APMeter.add (metrics.py:270-275, which calls that name without defining it) for instances that are DISJOINT on each side: predictions as a
 * label map (hdy_paste_label_map: -1 background, else the owning row) and truths as an instance map (the tile bank's uint16 map widened to
 * int32, or a slide map).  Mask IoU is then a sparse contingency count between two integer images: one streaming pass, integer-exact.
 *
 * hdy_label_overlap: pred_map, true_map int32 [elems] (64-bit count: a slide map may pass 2^31 entries), each read exactly once.  With
 * n_seg > 0 the maps are n_seg segments of seg_elems entries (elems = n_seg * seg_elems exactly; a batch of tile maps) and pred_base[s] /
 * true_base[s] (int32 [n_seg], ON THE DEVICE) are added to the non-negative labels of segment s, so tile-local rows become rows of the
 * concatenated arrays; n_seg = 0: one segment, no bases (both may be NULL).  A label that is negative, or outside [0, n_pred) / [0, n_true)
 * after the base, is background: any map content is memory-safe, and 0xFFFF of a widened uint16 map needs no rewrite while n_true <= 65535.
 *   pred_area[p] = entries whose prediction label is p; true_area[t] alike (int32, zeroed by the call);
 *   for every (p, t) that share at least one entry, inter(p, t) = the number of shared entries, in one slot of `table`:
 *     table = keys uint64 [slots] | counts uint32 [slots]; a used slot holds key = (p << 32 | t) and count = inter > 0, an unused one
 *     key = ~0 and count = 0.  slots is a power of two <= HDY_OVERLAP_MAX_SLOTS; table_bytes >= hdy_label_overlap_workspace_bytes(slots)
 *     (0 = slots invalid), 16-byte aligned.  The call initialises the table itself.  Which slot a pair occupies depends on arrival
 *     order; the SET of (p, t, inter) does not (integer adds), and that set is the result.
 *   status int32 [2] on the device = {pairs stored, inserts that found the table full}.  With status[1] != 0 the table is incomplete (areas
 *   are still exact); nothing is ever written outside the table.  The caller reads status once, when it wants to.
 *
 * hdy_mask_ap_match: the five rules of hdy_ap_match above, word for word, for ONE set of rows (rows of different images never share a pair, so
 * no offsets are needed), with rule 1's IoU taken from the table:
 *   union = area_p + area_t - inter in int64;  iou = float(inter) / float(union), one IEEE division of the two conversions
 * which is bit-identical to get_mask_ious on 0 / 1 fp32 masks while the counts stay below 2^24 (its "+ 1e-8" vanishes in fp32 once the union
 * is >= 1); above that each conversion rounds once, to nearest.  Rule 2: highest IoU, tie lowest truth row; rule 3: highest score, tie lower
 * prediction row; pred_row / true_row (int32, non-negative, distinct among rows that can meet; may be NULL) replace the positions.
 * table / slots as hdy_label_overlap left them, pred_area / true_area its areas; pred_scores fp32, labels int64; iouv (n_iou in [1, 16]),
 * pair_iou in (0, 1] and ignore (n_ignore in [0, 4]) are HOST values read before the call returns.  Outputs, one per prediction: hit (uint16
 * bits), live (uint8), match (int32 truth row or -1), match_iou (fp32).  Slots whose rows are out of range are skipped: any table content is
 * memory-safe.  workspace: 16-byte aligned, hdy_mask_ap_match_workspace_bytes(n_pred, n_true) (0 = a negative count), travels with its size.
 * Both: no allocation, no synchronisation, everything on `stream`; outputs are a pure function of the inputs (integer adds and 64-bit atomic
 * minima / maxima of distinct keys: no dependence on arrival order).  All argument checks are made before any launch: HDY_EINVAL + message. */
#define HDY_OVERLAP_MAX_SLOTS (1LL << 30)
size_t hdy_label_overlap_workspace_bytes(long long slots);
int hdy_label_overlap(const int* pred_map, const int* true_map, long long elems, long long seg_elems, int n_seg, const int* pred_base,
                      const int* true_base, int n_pred, int n_true, int* pred_area, int* true_area, void* table, size_t table_bytes,
                      long long slots, int* status, void* stream);
size_t hdy_mask_ap_match_workspace_bytes(int n_pred, int n_true);
int hdy_mask_ap_match(const void* table, size_t table_bytes, long long slots, const int* pred_area, const int* true_area, const float* pred_scores,
                      const long long* pred_labels, const int* pred_row, int n_pred, const long long* true_labels, const int* true_row, int n_true,
                      const float* iouv, int n_iou, float pair_iou, const long long* ignore, int n_ignore, unsigned short* hit, unsigned char* live,
                      int* match, float* match_iou, void* workspace, size_t ws_bytes, void* stream);

/* ---- mask branch primitives ------------------------------------------------------------
 * hdy_roi_align_fwd/bwd replace torchvision.ops.roi_align as the reference calls it (metayolo/models/yolo_head.py:243 on ground
 * truth boxes in training, :294 multiscale_roi_align on detections): feat NHWC [B][H][W][ldf] (C channels), rois [R][5] fp32
 * (image index, x1, y1, x2, y2 in input pixels), out NHWC [R][P][P][C]; sampling_ratio^2 bilinear samples per bin.
 * The backward scatters dout into dfeat_f32 [B][H][W][C] (fp32, zeroed by the caller) with atomic adds; hdy_cast_store moves
 * that image into a pitched gradient view (dst[m][c] (+)= src[m][c]).  hdy_relu_bwd: du = dz * (y > 0) for the head's
 * conv + bias + ReLU layers (torchvision MaskRCNNHeads / MaskRCNNPredictor, yolo_head.py:125-128). */
int hdy_roi_align_fwd(const void* feat, int ldf, int B, int H, int W, int C, const float* rois, int R, float spatial_scale, int P,
                      int sampling_ratio, int aligned, void* out, int dtype, void* stream);
int hdy_roi_align_bwd(const void* dout, float* dfeat_f32, int B, int H, int W, int C, const float* rois, int R, float spatial_scale, int P,
                      int sampling_ratio, int aligned, int dtype, void* stream);
/* hdy_roi_align_levels_fwd replaces multiscale_roi_align over a batch's detections (yolo_head.py:279-299, as compute_outputs calls it at
 * :320-353): per level `levels == l` -> nonzero -> roi_align -> cat -> reorder becomes ONE launch on the padded NMS result as hdy_nms_batched
 * leaves it.  levels: nl in [1, 8] records ON THE HOST, read before the call returns and passed to the kernel by value; level l is an NHWC map
 * [B][H][W][ldf] of C channels (C and dtype shared by all levels; ldf >= C, both multiples of the 16-byte vector: 4 fp32 / 8 bf16 channels).
 * boxes fp32 [B][max_det][4] xyxy in input pixels; level: the level id of each padded row as an fp32 value, row pitch nex floats (column 0 of
 * the NMS `extra` block); n_keep int32 [B] on the device, B in [1, 1024], each count clamped to [0, max_det].
 * out NHWC [out_rows][P][P][C] in COMPACTED order: image b's rows start at n_keep[0] + .. + n_keep[b - 1] and use image b of every map; the
 * kernel derives that prefix itself (as hdy_slide_append and hdy_det_outputs do), without atomics.  Row values: exactly hdy_roi_align_fwd on
 * the roi (b, box) with the level's map and spatial_scale — the two kernels share one device function, so the bits agree.  A row whose level
 * is not finite or not in [0, nl) is written as zeros (the rule of hdy_roi_align_fwd for an image index out of range).  Padded rows
 * >= n_keep[b] are scratch and never read.  Exactly min(out_rows, SUM n_keep) rows are written, nothing behind them.
 * HDY_EINVAL before any launch: null pointers (a level's map included), nl outside 1..8, B outside 1..1024, C not a multiple of the vector
 * width, P < 1, max_det < 1, nex < 1, out_rows < 0, misaligned out / boxes / maps.  out_rows == 0 launches nothing.
 *
 * hdy_mask_rows is the channel choice that follows the mask head (yolo_head.py:346-351: `masks[arange, mask_labels][:, None]`, rows with a
 * negative mask label zeroed), for all rows at once: vals fp32 [R][M][M] with channel pitch ldv >= K (the head's sigmoid), labels int64 [R],
 * mask_indices int32 [n_idx] on the device;  out fp32 [R][1][M][M] contiguous, out_elems = R * M * M exactly (else HDY_EINVAL):
 *   idx = mask_indices[max(labels[r], 0)];  out[r] = vals[r][:][:][idx], or zeros when idx < 0.
 * Pure data movement: the values are copied bit for bit.  mask_indices_host (may be NULL): the same table on the host; with it an idx >= K is
 * HDY_EINVAL before the launch.  Whatever the host cannot see (a label >= n_idx, an idx >= K in a device-only table) writes a row of zeros:
 * the kernel never reads out of range. */
typedef struct hdy_roi_level {
    const void* feat;
    int H, W, ldf;
    float spatial_scale;
} hdy_roi_level;
int hdy_roi_align_levels_fwd(const hdy_roi_level* levels, int nl, int C, const float* boxes, const float* level, int nex, const int* n_keep, int B,
                             int max_det, int P, int sampling_ratio, int aligned, void* out, int out_rows, int dtype, void* stream);
int hdy_mask_rows(const float* vals, int ldv, int K, const long long* labels, const int* mask_indices, const int* mask_indices_host, int n_idx, int R,
                  int M, float* out, long long out_elems, void* stream);
int hdy_relu_bwd(const void* dz, const void* y, void* du, long long n, int dtype, void* stream);
int hdy_cast_store(const float* src, void* dst, int ldd, long long M, int C, int accumulate, int dtype, void* stream);

/* ---- fused detection loss --------------------------------------------------------------
 * Replaces Detect.matcher (metayolo/models/yolo_head.py:358-417), DetLoss.forward (metayolo/models/loss.py:190-244) with
 * bbox_iou(CIoU) (metayolo/models/utils_general.py:193-231) and their autograd backward: target assignment, CIoU box loss,
 * objectness / class BCE, and the gradient w.r.t. the logits, written into the NHWC buffers the backward plan consumes.
 * logits[l]: fp32 [B][ny][nx][ldl], channel a*no+o;  gdet[l]: dtype [B][ny][nx][ldg] (ldl, ldg multiples of 4, 16-byte aligned
 * bases; channels >= na*no of gdet are written as zero);  anchors_grid: nl*na*2 HOST floats in grid
 * units; balance: nl HOST floats; gts: device [nt][5] (img, cx, cy, w, h normalised); tcls: device [nt][nc] class targets;
 * cls_cw: nc HOST floats.  out: device [4] = loss (x batch), box, obj, cls items.  hdy_det_loss: BCE class / objectness terms with one
 * class pos_weight, the reference's default objectness target (gr = 1, no sort_obj_iou); no autobalance.
 * workspace: hdy_det_loss_workspace_bytes(..., nt) bytes for calls with up to nt targets (sums, one list head per cell and anchor,
 * one record per possible match: nl * 5 * na * nt of them). */
size_t hdy_det_loss_workspace_bytes(int nl, const int* ny, const int* nx, int B, int na, int nc, int nt);
int hdy_det_loss(const float* const* logits, int ldl, void* const* gdet, int ldg, int dtype, const int* ny, const int* nx, int nl, int B,
                 int na, int nc, const float* anchors_grid, const float* balance, const float* gts, const float* tcls, int nt,
                 const float* cls_cw, float cls_pw, float obj_pw, float anchor_t, float label_smoothing, float h_box, float h_obj, float h_cls,
                 float* out, void* workspace, size_t ws_bytes, void* stream);
/* hdy_det_loss with the other DetLoss forms (metayolo/models/loss.py:68-94 FocalLoss, :150 gr, :212-217 sort_obj_iou); hdy_det_loss is
 * this call with the BCE form and gives the same bits.  cls_pw: nc HOST floats (per-class pos_weight).  fl_gamma > 0: both BCE terms
 * wrapped in FocalLoss(gamma = fl_gamma, alpha = fl_alpha); fl_gamma == 0: BCE (fl_alpha unused).  gr < 1: a matched cell's objectness
 * target is (1 - gr) + gr * iou; sort_obj_iou != 0: a cell matched several times keeps its largest iou instead of its last candidate's.
 * HDY_EINVAL before any device work when fl_gamma is negative or not finite, or fl_alpha or gr is not finite. */
int hdy_det_loss_ex(const float* const* logits, int ldl, void* const* gdet, int ldg, int dtype, const int* ny, const int* nx, int nl, int B,
                    int na, int nc, const float* anchors_grid, const float* balance, const float* gts, const float* tcls, int nt,
                    const float* cls_cw, const float* cls_pw, float obj_pw, float anchor_t, float label_smoothing, float h_box, float h_obj,
                    float h_cls, float fl_gamma, float fl_alpha, float gr, int sort_obj_iou, float* out, void* workspace, size_t ws_bytes,
                    void* stream);
/* Which matched cell of each target feeds the mask branch (metayolo/models/yolo_head.py:231-262: per target the matched cell whose decoded
 * box has the best IoU with the truth — first in the reference's row order on ties — kept when that IoU >= min_iou = 0.8).  Same logits /
 * geometry / anchors_grid / gts / anchor_t as hdy_det_loss, anchors_px [nl][na][2] and strides [nl] as hdy_decode.  Device outputs:
 * counts [1 + nl] (kept, kept per level), keep_t [nt] int64 target of kept row k (target order), rois [nl][nt][5] (image, x1, y1, x2, y2 of
 * the TRUTH in input pixels, compact per level), order [nt] int64 = position of kept row k in the level-by-level concatenation.
 * workspace: nt * 16 bytes, 8-byte aligned. */
int hdy_mask_select(const float* const* logits, int ldl, const int* ny, const int* nx, int nl, int B, int na, int no, const float* anchors_grid,
                    const float* anchors_px, const float* strides, const float* gts, int nt, float anchor_t, float min_iou, int* counts,
                    long long* keep_t, float* rois, long long* order, void* workspace, size_t ws_bytes, void* stream);
/* gts / tcls of hdy_det_loss from the batch's annotations (replaces the xyxy -> xywh conversion and the one-hot encoding of
 * Detect.forward's target preparation, metayolo/models/yolo_head.py:217-222: ~15 eager tensor ops per step): boxes device [nt][4] corner boxes
 * (normalised, already clamped to [0, 1]), img device [nt] image index of each row (fp32), labels device [nt] int64 class labels
 * 1..nc (anything else: no class) -> gts [nt][5], tcls [nt][nc]. */
int hdy_det_targets(const float* boxes, const float* img, const long long* labels, int nt, int nc, float* gts, float* tcls, void* stream);
int hdy_scale_inplace(void* p, long long n, const float* scale_dev, int dtype, void* stream);

/* ---- Semantic-segmentation branch (hnet's PanopticSeg) ---------------------------------------------
 * Replaces, under autograd, torch.nn.GroupNorm(32, C) + ReLU and nn.Upsample(scale_factor=2, mode='bilinear', align_corners=True)
 * of PanopticFeatureConnector (hnet/segmentation/utils_seg.py:21-36), the branch sum (:58), nn.Upsample / F.interpolate(...,
 * align_corners=True) and torch.nn.Softmax2d of PanopticSeg (hnet/segmentation/panoptic_seg.py:13-19,38-39) and its soft-dice
 * criterion (:22,40; `SoftDiceLoss` is not defined anywhere upstream: restated from the repository's own dice, mask_iou(factor=0),
 * metayolo/models/utils_general.py:268-280).  NHWC, pixel pitches, caller-owned workspaces as everywhere else. */
size_t hdy_groupnorm_workspace_floats(int N, int C);
int hdy_groupnorm_fwd(const void* x, int ldx, const float* gamma, const float* beta, void* y, int ldy, float* stat, float* ab, int N, int HW,
                      int C, int G, float eps, int relu, int dtype, float* workspace, size_t ws_floats, void* stream);
int hdy_groupnorm_bwd(const void* dout, int lddo, const void* x, int ldx, const float* gamma, const float* stat, const float* ab, void* dx, int lddx,
                      float* dgamma, float* dbeta, int accumulate, float* coef, int N, int HW, int C, int G, int relu, int dtype, float* workspace,
                      size_t ws_floats, void* stream);
int hdy_bilinear_fwd(const void* x, int ldx, void* y, int ldy, int N, int Hi, int Wi, int Ho, int Wo, int C, int accumulate, int dtype, void* stream);
int hdy_bilinear_bwd(const void* dy, int lddy, void* dx, int lddx, int N, int Hi, int Wi, int Ho, int Wo, int C, int accumulate, int dtype, void* stream);
/* one axis of the same (the resize is separable): tensors [outer][Ao -> Ai][inner][ld]; W pass outer = N*Ho, inner = 1, then H pass outer = N,
 * inner = Wi over the W pass's result — 8x fewer candidate reads than the 2-D gather at the x8 resize of the segmentation logits */
int hdy_bilinear_bwd_axis(const void* dy, int lddy, void* dx, int lddx, long long outer, int Ai, int Ao, int inner, int C, int accumulate, int dtype,
                          void* stream);
size_t hdy_softdice_workspace_floats(int N, int nc);
int hdy_softdice(const float* logits, int ldl, const float* targets, const float* class_weight, int N, int HW, int nc, float* loss,
                 const float* upstream, float* dlogits, int lddl, float* workspace, size_t ws_floats, void* stream);
/* hdy_softdice's loss, and its gradient already reduced along W by the transposed resize (the W pass of hdy_bilinear_bwd_axis) without the
 * full-resolution gradient tensor: logits fp32 [N][H][W][4] with nc <= 4 classes (the segmentation header's resized class logits,
 * hnet/segmentation/panoptic_seg.py:37-40), dw [N][H][Wi][4]; the caller finishes with the H pass.  Bit-identical to the two-call path.
 * workspace: ws_floats >= hdy_softdice_workspace_floats(N, nc) (every workspace of this section: HDY_EINVAL when smaller). */
int hdy_softdice_wgrad(const float* logits, const float* targets, const float* class_weight, int N, int H, int W, int nc, int Wi, float* loss, float* dw,
                       float* workspace, size_t ws_floats, void* stream);
int hdy_softmax2d(const float* logits, int ldl, float* probs, int ldp, long long M, int nc, void* stream);

/* The stem's weight gradient (layers.py:31 Conv(3, c, 6, 2, 2), backward of train.py:472) with the BatchNorm / SiLU backward of its unit applied
 * while the gradient tile is staged: dz = gradient of the unit's activation output, y = its raw conv output, c1 / c2 from
 * hdy_bn_act_bwd(dy = NULL).  The stem has no data gradient, so its dy is never written.  x = the hdy_stem_prep buffer; bf16; K in
 * {16, 32, 64}; workspace as hdy_conv_wgrad_workspace_bytes(..., stem = 1). */
int hdy_conv_wgrad_stem_fused_ok(int N, int H, int W, int K);
int hdy_conv_wgrad_stem_fused(const void* x, const void* dz, int lddz, const void* y, int ldy, const float* scale, const float* shift, const float* mean,
                              const float* invstd, const float* c1, const float* c2, int N, int H, int W, int K, float* grad_a, int K_a, float* grad_b,
                              int K_b, int accumulate, void* workspace, size_t ws_bytes, void* stream);

/* ---- SyncBatchNorm (reference: train.py:281-283, torch.nn.SyncBatchNorm.convert_sync_batchnorm when --sync-bn).  sums = 2*K + 1 doubles:
 * [SUM x | SUM x^2 | element count].  Forward: hdy_bn_slab_sums over the conv's statistic slabs -> all-reduce(sums) by the caller ->
 * hdy_bn_finalize_sums (same outputs and running-statistic update as hdy_bn_finalize[_pair]; sums may point at a channel slice of a
 * wider [2][sums_ld] block, count at its 2*sums_ld-th double; Ka == K: one module).  Backward: hdy_bn_act_bwd[_pair] with dy == NULL (local statistics, local dgamma / dbeta) -> hdy_bn_slab_sums over its
 * workspace partials (hdy_bn_bwd_blocks(M) slabs of [2][K]) -> all-reduce -> hdy_bn_bwd_coeffs_sums -> hdy_bn_act_bwd_apply. */
int hdy_bn_slab_sums(const float* slabs, int slab_ld, int nslabs, int K, long long count, double* sums, void* stream);
int hdy_bn_finalize_sums(const double* sums, int sums_ld, const double* count, int K, int Ka, const float* gamma_a, const float* beta_a, float* running_mean_a, float* running_var_a,
                         const float* gamma_b, const float* beta_b, float* running_mean_b, float* running_var_b, float eps, float momentum,
                         float* scale, float* shift, float* save_mean, float* save_invstd, void* stream);
int hdy_bn_bwd_coeffs_sums(const double* sums, int K, float* c1, float* c2, void* stream);

/* ---- optimizer step of the training loop and the weight EMA in one launch: SGD | Adam | AdamW (reference: train.py:208-233 builds one of the
 * three over three parameter groups, stepped at train.py:478; :249 / :480 ModelEMA.update after every optimizer step,
 * metayolo/common.py:128-155).  One launch for all tensors: a device table of descriptors, first_block = running sum of hdy_opt_blocks(n),
 * a block owns 4096 consecutive elements of one row.  A row: fp32 parameter p; gradient g or NULL; first state m (SGD momentum buffer / Adam
 * exp_avg) or NULL; second state v (Adam exp_avg_sq) or NULL; EMA destination or NULL; first = m / v are uninitialised: written, not read (as
 * from zeros for Adam, buf = g' for SGD).  g == NULL: an EMA-only row — p, m, v are not written, ema is updated from p (BatchNorm running
 * statistics, frozen and gradient-less parameters).  A row with g and ema both NULL is a caller error (nothing is written for it).  16-byte
 * accesses when all of a row's pointers are 16-byte aligned and n % 4 == 0, scalar ones otherwise.
 *   algo: one of HDY_OPT_* for the whole table.
 *     SGD: torch.optim.SGD, g' = g + wd*p; buf = momentum*buf + (1-dampening)*g'; p -= lr * (nesterov ? g' + momentum*buf : buf); m == NULL:
 *     no momentum, p -= lr*g'.  Adam / AdamW: torch.optim.adam's single-tensor path,
 *     AdamW: p *= 1 - lr*wd;  Adam: g += wd*p;  m += (g - m)*(1 - beta1);  v = beta2*v + (1 - beta2)*g*g;
 *     p -= (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps),  bc1 = 1 - beta1^step, bc2 = 1 - beta2^step,
 *     with fused multiply-adds and correctly rounded division and square root.
 *   hyper: HOST array of nslots (<= HDY_OPT_MAX_SLOTS) rows of HDY_OPT_HYPER floats, passed by value to the kernel; a slot is one (parameter
 *     group, step count) pair and a row names its slot.  SGD: {lr, weight_decay, momentum, dampening};  Adam / AdamW: {lr / bc1,
 *     Adam: weight_decay | AdamW: 1 - lr*weight_decay, 1 - beta1, beta2, 1 - beta2, sqrt(bc2), eps}, each computed in double and rounded once.
 *   has_ema != 0: rows with an EMA destination get ema = ema_decay * ema + ema_one_minus_decay * (the parameter value just written, or p
 *     itself on an EMA-only row); has_ema == 0: the ema column is ignored.  nesterov: SGD only. */
#define HDY_OPT_MAX_SLOTS 16
#define HDY_OPT_HYPER 8
#define HDY_OPT_SGD 0
#define HDY_OPT_ADAM 1
#define HDY_OPT_ADAMW 2
typedef struct hdy_opt_desc {
    float* p;
    const float* g;
    float* m;
    float* v;
    float* ema;
    long long n;
    int slot, first, first_block, pad_;
} hdy_opt_desc;
int hdy_opt_blocks(long long n);
int hdy_opt_step(const hdy_opt_desc* table_device, int ndesc, int total_blocks, int algo, int nesterov, const float* hyper, int nslots, int has_ema,
                 float ema_decay, float ema_one_minus_decay, void* stream);

/* ---- launch-list executor (csrc/exec.hip): one call issues a whole precomputed list of launches on two streams — a plan's forward or backward
 * list, whose pointers, shapes and order are fixed (no reference counterpart: the order is the one PyTorch's autograd engine gives the same work,
 * train.py:472).  program = 64-bit words, per item [op][nargs][arg 0]..[arg nargs-1]:
 *   op = hdy_exec_op("hdy_...") (>= 0; -1: that entry point cannot be listed): the entry point's parameters in order WITHOUT the trailing
 *        stream, each widened to 64 bits (pointers / integers by value, float / double by bit pattern);
 *   op = HDY_EXEC_FORK, args {token, words}: the next `words` words run on side_stream once everything issued so far on main_stream is done;
 *   op = HDY_EXEC_JOIN, args {token}: main_stream waits for the launches of that fork (a token never forked: no wait).
 * Tokens are < 65536; their events live per device for the life of the process.  Returns the first non-zero status of a listed entry point
 * (hdy_last_error names it), HDY_EINVAL for a malformed program.  hdy_exec_join: the join alone, for a caller that runs the rest of a
 * list itself.  hdy_copy_f32: dst[0..n) = src[0..n) on the stream (a list item in place of a host-side tensor copy). */
#define HDY_EXEC_FORK 0xF0F0F0F0ull
#define HDY_EXEC_JOIN 0xF0F0F0F1ull
int hdy_exec_op(const char* name);
int hdy_exec_run(const unsigned long long* program, size_t nwords, void* main_stream, void* side_stream);
int hdy_exec_join(unsigned long long token, void* main_stream);
int hdy_copy_f32(const float* src, float* dst, long long n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HDYOLO_H */
