/* cmx_mlp.h — C-ABI of libcmx_hip.so, part 6: the Mix-FFN of stages 1-2 (dual_segformer.py:67-74) with the Linear on
 * either side of the depthwise 3x3 conv computed inside the conv's launch (csrc/dwconv.hip).  The conventions, the
 * status codes, CMX_ABI_VERSION and hipStream_t are cmx_hip.h's; the Python binding parses this file as it parses that
 * one (every declaration on one line) and keeps its entry points in a table of their own (_lib.MLP_SIGNATURES).
 */
#ifndef CMX_MLP_H
#define CMX_MLP_H
#include "cmx_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* 16-bit dtypes, C = 64 or 128 (K of both Linears), hidden % 64 == 0, act = GELU; anything else is CMX_ERR_SHAPE.
 * Results are bit-identical to the two launches each entry point replaces.
 *   fc1_dwconv_fwd = cmx_gemm (f0 = x W1^T + b1) then cmx_dwconv3x3_fwd_save on f0.  x (NI*H*W, C) rows, W1 (G, hidden, C),
 *      b1 (G, hidden), all contiguous; w (G, hidden, 9), b (G, hidden) the depthwise taps and bias; f0, out, gprime
 *      (NI, H, W, hidden): f0 is written too (the backward and fc1's weight gradient read it).
 *   fc2_dwconv_bwd = cmx_gemm (da = dz W2) then cmx_dwconv3x3_bwd_saved on da, which is never written.  dz (NI*H*W, C)
 *      rows = fc2's output gradient, W2 (G, C, hidden) contiguous, h = f0; dh, dw, db, workspace
 *      (cmx_dwconv3x3_bwd_workspace of the hidden width) and the partials left with dw = db = NULL as bwd_saved. */
int cmx_mlp_fc1_dwconv_fwd(const void* x, const void* W1, const float* b1, const float* w, const float* b, void* f0, void* out, void* gprime, int NI, int imgs_per_group, int H, int W, int C, int hidden, int act, int dtype, hipStream_t stream);
int cmx_mlp_fc2_dwconv_bwd(const void* dz, const void* W2, const void* h, const void* gprime, const float* w, void* dh, float* dw, float* db, float* workspace, int NI, int imgs_per_group, int H, int W, int C, int hidden, int accumulate, int dtype, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif
