/* cmx_fcn.h — C-ABI of libcmx_hip.so, part 4: the fused final upsample + loss at the scales of an FCN head (the
 * FCN-32s decode head on the stage-4 map, the auxiliary head on the stage-3 map).  The conventions, the status codes,
 * CMX_ABI_VERSION and hipStream_t are cmx_hip.h's; the Python binding parses this file as it parses that one (every
 * declaration on one line) and keeps its entry points in a table of their own (_lib.FCN_SIGNATURES).
 */
#ifndef CMX_FCN_H
#define CMX_FCN_H
#include "cmx_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- fused bilinear upsample by S (align_corners=False, torch's clamped border taps) + loss, S in {8, 16, 32}, in
 *      the one-pass training form of cmx_upsample_loss_fwd_adj.  logits (B, h, w, K) in `dtype`, label (B, S h, S w)
 *      int64, K <= 40.  kind -1: nn.CrossEntropyLoss(mean, ignore_index) (class_weight NULL); kinds 0, 1, 2 and their
 *      parameters: exactly cmx_upsample_loss_fwd_adj's (cmx_hip.h), normalisers, label clamping of kind 2, the
 *      gamma == 0 or gamma >= 1 rule and NaN against 0 when nothing is valid included.
 *      out (3) fp32 = [loss, 1 / norm, norm]; adj (B, h, w, K) fp32 = the unscaled bilinear adjoint of the per-pixel
 *      dl/dz: the backward is cmx_upsample_ce_bwd_scale.
 *      For a power-of-two S every interpolation weight is a multiple of 1 / (2S): exact in fp32.  The S x S pixels
 *      [S r - S/2, S r + S/2) x [S c - S/2, S c + S/2) (a "cell"; r in [0, h], c in [0, w], clipped at the image)
 *      read the four low-res pixels (r - 1 .. r, c - 1 .. c) and no other, so a cell's gradient has an adjoint on
 *      those four only.  Launches: the cells kernel (loss partials per workgroup, and per cell its four corner sums,
 *      K floats each, in the workspace), a gather that adds each low-res pixel's four corner sums in one fixed order
 *      into adj, and the finalize.  No full-resolution tensor is written and the labels are read once; no
 *      floating-point atomic: bit-identical from run to run; nothing is read back to the host.
 *      workspace: cmx_upsample_loss_scaled_workspace bytes = (2 per workgroup + B (h + 1) (w + 1) x 4 x 40) fp32;
 *      0 for a shape the entry point refuses.
 *      S outside {8, 16, 32}, K outside 1..40, B, h or w <= 0: CMX_ERR_SHAPE.  A NULL operand, a base that is not
 *      aligned to its element, kind outside -1..2, kind 2 with 0 < gamma < 1 or gamma < 0 or NaN, a class_weight
 *      with kind 2 or kind -1: CMX_ERR_ARG.  An unknown dtype: CMX_ERR_DTYPE. */
size_t cmx_upsample_loss_scaled_workspace(int B, int h, int w, int S);
int cmx_upsample_loss_scaled_fwd_adj(const void* logits, const int64_t* label, const float* class_weight, float* adj, float* out, float* workspace, int B, int h, int w, int S, int K, int ignore_index, int kind, float gamma, float alpha, float ce_scale, float focal_scale, int dtype, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif
