/* cmx_easpp.h — C-ABI of libcmx_hip.so, part 3: the eASPP neck of the mit_b*_w_ef_aspp backbones
 * (models/encoders/dual_segformer_w_ef_aspp.py:18-157).  The conventions, the status codes, CMX_ABI_VERSION and
 * hipStream_t are cmx_hip.h's; the Python binding parses this file as it parses that one (every declaration on one
 * line) and keeps its entry points in a table of their own (_lib.EASPP_SIGNATURES).
 */
#ifndef CMX_EASPP_H
#define CMX_EASPP_H
#include "cmx_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- grouped dilated 3x3 convolution, C -> C channels with C == 64 (anything else: CMX_ERR_SHAPE), stride 1,
 *      dilation = padding = rate, no bias (ASPPConv.block[0], :22): ONE launch runs the three branches of one depth
 *      level, group g on its own input, weight and output.  Activations are token-major NHWC rows (B*h*w of them)
 *      of C channels with a row stride in elements (>= C, a multiple of 16 bytes; bases 16-byte aligned); weights
 *      are the flat store's tap-major (Cout, kh, kw, Cin).  fp32 accumulation on MFMA for all three dtypes (fp32:
 *      the exact 32x32x2 form).  Zero padding: a source pixel outside the map contributes nothing, and a tap whose
 *      offset (ky - 1, kx - 1) * rate leaves the map for EVERY pixel (|dy| >= h or |dx| >= w) is skipped as a whole,
 *      which is exact.  No im2col buffer, no workspace.
 *      fwd:   y_g[p][co]  = sum_tap sum_ci x_g[p + off(tap)][ci] * w_g[co][tap][ci]
 *      dgrad: dx_g[p][ci] = sum_tap sum_co dy_g[p - off(tap)][co] * w_g[co][tap][ci]   (mirrored taps, w transposed)
 *      wgrad: dw_g[co][tap][ci] = sum_p dy_g[p][co] * x_g[p + off(tap)][ci], fp32, OVERWRITTEN (a skipped tap is
 *             written as zeros).  Chunks of 128 rows per workgroup; with more than one chunk the per-workgroup
 *             partials go to `workspace` (cmx_easpp_conv_wgrad_workspace bytes) and a second launch folds them in
 *             chunk order: no float atomics, bit-identical from run to run.
 *      A NULL operand, a rate < 1, a misaligned base or stride: CMX_ERR_ARG; B, h, w <= 0 or C != 64: CMX_ERR_SHAPE. */
int cmx_easpp_conv_fwd(const void* x0, const void* x1, const void* x2, const void* w0, const void* w1, const void* w2, void* y0, void* y1, void* y2, int B, int h, int w, int C, int r0, int r1, int r2, int64_t ldx, int64_t ldy, int dtype, hipStream_t stream);
int cmx_easpp_conv_dgrad(const void* dy0, const void* dy1, const void* dy2, const void* w0, const void* w1, const void* w2, void* dx0, void* dx1, void* dx2, int B, int h, int w, int C, int r0, int r1, int r2, int64_t lddy, int64_t lddx, int dtype, hipStream_t stream);
size_t cmx_easpp_conv_wgrad_workspace(int B, int h, int w);
int cmx_easpp_conv_wgrad(const void* dy0, const void* dy1, const void* dy2, const void* x0, const void* x1, const void* x2, float* dw0, float* dw1, float* dw2, float* workspace, int B, int h, int w, int C, int r0, int r1, int r2, int64_t lddy, int64_t ldx, int dtype, hipStream_t stream);

/* ---- the concat buffer (:152) and the pooled branch's broadcast (AsppPooling, :41-45: bilinear align_corners=True
 *      of a 1x1 map is a broadcast).  cat (B*N, 5*Cm) = [y0 | y1 | y2 | y3 | pool[b] on every row of image b], y_i
 *      (B*N, Cm) contiguous in the storage dtype, pool (B, Cm) fp32; Cm % 64 == 0.  The entry points take no strides:
 *      the caller passes contiguous tensors (the Python wrappers check it); y_i, cat, d_i, dcat and pool_bwd's dx
 *      off a 16-byte boundary are refused with CMX_ERR_ARG.
 *      bwd: d_i = dcat's column slot i, dpool[b][c] = sum_n dcat[b*N + n][4*Cm + c] (fp32, rows summed in a fixed
 *      order), in one launch.
 *      pool_bwd: the adjoint of nn.AdaptiveAvgPool2d(1): dx[b*N + n][c] = (1/N) sum_s dpooled_part[s*slice_stride +
 *      b*C + c], dpooled given as the nslice (<= 16) dx slices of cmx_small_linear_bwd. */
int cmx_easpp_concat_fwd(const void* y0, const void* y1, const void* y2, const void* y3, const float* pool, void* cat, int B, int N, int Cm, int dtype, hipStream_t stream);
int cmx_easpp_concat_bwd(const void* dcat, void* d0, void* d1, void* d2, void* d3, float* dpool, int B, int N, int Cm, int dtype, hipStream_t stream);
int cmx_easpp_pool_bwd(const float* dpooled_part, int nslice, int64_t slice_stride, void* dx, int B, int N, int C, int dtype, hipStream_t stream);

/* ---- the elementwise nn.Dropout(p) of eASPP.project (:126) as a scale for cmx_bn_apply's dscale with
 *      rows_per_sample = 1: dscale[i] = (u >= p) / (1 - p), u = splitmix64(seed, state[0], i), cmx_step_masks's
 *      generator.  state: two uint64 owned by the caller, both zero at first: state[0] is the step, advanced on the
 *      device by the last workgroup to finish (every workgroup has read it by then), so a replayed HIP graph draws a
 *      fresh mask; state[1] is that arrival counter (left at zero).  0 <= p < 1, n > 0, else CMX_ERR_ARG. */
int cmx_easpp_dropout_mask(float* dscale, int64_t n, float p, uint64_t seed, uint64_t* state, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif
