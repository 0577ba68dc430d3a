/* cmx_ohem.h — C-ABI of libcmx_hip.so, part 2: ProbOhemCrossEntropy2d on the fused final upsample + loss
 * path and its device-side select.  The conventions, the status codes, CMX_ABI_VERSION and hipStream_t
 * are cmx_hip.h's; the Python binding parses this file as it parses that one (every declaration on one
 * line) and keeps its entry points in a table of their own (_lib.OHEM_SIGNATURES).
 */
#ifndef CMX_OHEM_H
#define CMX_OHEM_H
#include "cmx_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- fused final upsample + ProbOhemCrossEntropy2d(thresh, min_kept) (utils/loss_opr.py:205-255; reduction 'mean',
 *      no class weight; H = 4h, W = 4w, K <= 40, else CMX_ERR_SHAPE), in the training form of
 *      cmx_upsample_ce_fwd_adj.  With p_y the target-class probability of a valid pixel (label != ignore_index and
 *      0 <= label < K; any other label counts as ignored, as plain CE does):
 *        min_kept <= 0 or min_kept > n_valid: nothing is dropped, threshold = +inf, the result is plain CE (nothing
 *          valid: loss NaN, zero gradient);
 *        otherwise threshold = max(thresh, the min_kept-th smallest p_y), kept = valid and p_y <= threshold (every tie
 *          at the threshold is kept, so n_kept may exceed min_kept);
 *        loss = mean over kept of -log p_y, gradient (p - onehot) / n_kept at kept pixels and 0 elsewhere.
 *      Launch sequence, nothing read back to the host (graph-capturable, the regime is chosen on the device): a
 *      launch that zeroes the select's workspace; a statistics pass that writes py (B, H, W) fp32 = p_y, 2.0 at a
 *      pixel that is not valid, and counts n_valid and n_below = #(p_y <= thresh) with integer atomics; the select
 *      (below) on py; the gradient pass = plain CE's forward with every pixel whose stored py exceeds the device
 *      scalar threshold ignored (it recomputes no probability for the decision: the two passes agree by
 *      construction); the finalize.
 *      out (4) fp32 = [loss, 1 / n_kept, n_kept, threshold]; counts (3) = [n_valid, n_below, n_kept]; adj (B, h, w, K)
 *      fp32 = the unscaled bilinear adjoint of (p - onehot) at the kept pixels: the backward is
 *      cmx_upsample_ce_bwd_scale, which reads out[1].  NaN thresh, a NULL operand: CMX_ERR_ARG.  No floating-point
 *      atomic anywhere: bit-identical from run to run.
 *      cmx_ohem_select: the select alone, on n keys py (a key is valid when its bit pattern is below that of 2.0f, i.e.
 *      0 <= key < 2; anything else -- the 2.0 sentinel, negatives, NaN -- is not).  It counts n_valid and n_below
 *      itself, then runs what the fused entry point runs: a radix select on the keys' bit patterns (a non-negative
 *      float orders as its uint32) in three digit passes of 11, 11 and 10 bits, integer histograms privatised in LDS
 *      and merged with integer atomics, every dependency between blocks a kernel boundary.  The k-th value is exact
 *      on the stored fp32 keys.  When n_below >= min_kept the threshold is thresh and the digit passes return at
 *      once (they are launched all the same: no host branch).  threshold: one float; n <= 0 or n >= 2^31, NaN
 *      thresh, a NULL operand: CMX_ERR_ARG.  workspace: cmx_ohem_select_workspace bytes (two counters and the three
 *      histograms); cmx_upsample_ohem_workspace adds 2 fp32 loss partials per block of the 6 x 8 low-res tiling. */
size_t cmx_ohem_select_workspace(int64_t n);
int cmx_ohem_select(const float* py, int64_t n, float thresh, int min_kept, float* threshold, int64_t* counts, void* workspace, hipStream_t stream);
size_t cmx_upsample_ohem_workspace(int B, int h, int w);
int cmx_upsample_ohem_fwd_adj(const void* logits, const int64_t* label, float* adj, float* out, float* py, int64_t* counts, void* workspace, int B, int h, int w, int H, int W, int K, int ignore_index, float thresh, int min_kept, int dtype, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif
