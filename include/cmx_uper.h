/* cmx_uper.h — C-ABI of libcmx_hip.so, part 7: what the UPerNet decode head (models/decoders/UPernet.py) needs beyond
 * the GEMM family and the BatchNorm kernels: the pyramid pooling, the align_corners=False upsample + concat of several
 * sources, the top-down upsample + add, and the weight flip that turns a stride-1 convolution's input gradient into
 * one cmx_conv_implicit_fwd launch.  The conventions, the status codes, CMX_ABI_VERSION and hipStream_t are
 * cmx_hip.h's; the Python binding parses this file as it parses that one (every declaration on one line) and keeps
 * its entry points in a table of their own (_lib.UPER_SIGNATURES).
 *
 * Common to every entry point: activations are token-major NHWC rows in the storage dtype (0 fp32, 1 bf16, 2 fp16),
 * arithmetic is fp32 and each output element is rounded once; bases are 16-byte aligned and channel counts are
 * multiples of 8.  A NULL operand or a misaligned base / stride: CMX_ERR_ARG; a shape outside the stated one:
 * CMX_ERR_SHAPE; an unknown dtype: CMX_ERR_DTYPE; a refused call launches nothing.  No float atomics and every sum in
 * a fixed order: bit-identical from run to run.  No host synchronisation.
 */
#ifndef CMX_UPER_H
#define CMX_UPER_H
#include "cmx_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- pyramid pooling (PPM, UPernet.py:107-146): nn.AdaptiveAvgPool2d(s) of x (B*h*w, C) at up to four scales in ONE
 *      launch.  s0 is 1..8; s1..s3 are 1..8, or 0 from the first absent scale on.  pooled (B * sum s_k^2, C): block k
 *      starts at row B * sum_{j<k} s_j^2 and holds (B, s_k, s_k, C).  Bin (i, j) covers rows [floor(i h / s),
 *      ceil((i + 1) h / s)) and columns likewise (torch's rule: bins overlap when s does not divide h and repeat
 *      pixels when h < s); its value is the fp32 sum of its pixels in row-major order divided by their count.
 *      bwd, a gather in one launch: dx[p] = add[p] + sum_k sum_{bins of scale k that hold p} dpooled[bin] / count(bin),
 *      scales, bin rows and bin columns in ascending order.  add (B*h*w rows of C at row stride ldadd elements, a
 *      multiple of 8; NULL: absent) is the gradient that reaches x by another way: the head passes the first C columns
 *      of the PPM concat's gradient. */
int cmx_ppm_pool_fwd(const void* x, void* pooled, int B, int h, int w, int C, int s0, int s1, int s2, int s3, int dtype, hipStream_t stream);
int cmx_ppm_pool_bwd(const void* dpooled, const void* add, int64_t ldadd, void* dx, int B, int h, int w, int C, int s0, int s1, int s2, int s3, int dtype, hipStream_t stream);

/* ---- torch.cat([skip, up(src_0), ..., up(src_{n-1})], 1) with up = F.interpolate(., (H, W), mode='bilinear',
 *      align_corners=False) (UPernet.py:58-66, :94-100) in one launch: cat (B*H*W, Cs + n*C), skip (B*H*W, Cs), src_i
 *      (B*h_i*w_i, C), all contiguous, n = 1..4 (the sources past n are ignored), any h_i, w_i >= 1: a source larger
 *      than (H, W) is resampled down by the same rule (the PPM's 6 x 6 branch on a smaller stage-4 map).  Cs = 0
 *      (skip then ignored) is allowed.  The weight rule is cmx_bilinear_fwd_nhwc's (torch's, in fp32):
 *      src = max((Y + 0.5) h / H - 0.5, 0), y0 = floor(src), y1 = min(y0 + 1, h - 1), lambda = src - y0.
 *      bwd, one launch: dskip (NULL: not written) = dcat's columns [0, Cs); dsrc_i[b][r][c][:] = sum_Y sum_X wy(Y, r)
 *      wx(X, c) dcat[b][Y][X][Cs + i C :][:C], a gather over the output pixels whose taps touch (r, c), with the
 *      forward's own indices and weights (an exact adjoint whatever the rounding of src), rows dealt to four waves
 *      whose sums are added in wave order.  No workspace. */
int cmx_upcat_multi_fwd(const void* skip, const void* src0, const void* src1, const void* src2, const void* src3, void* cat, int B, int H, int W, int Cs, int C, int n, int h0, int w0, int h1, int w1, int h2, int w2, int h3, int w3, int dtype, hipStream_t stream);
int cmx_upcat_multi_bwd(const void* dcat, void* dskip, void* dsrc0, void* dsrc1, void* dsrc2, void* dsrc3, int B, int H, int W, int Cs, int C, int n, int h0, int w0, int h1, int w1, int h2, int w2, int h3, int w3, int dtype, hipStream_t stream);

/* ---- the top-down step laterals[i-1] + F.interpolate(laterals[i], ., mode='bilinear', align_corners=False)
 *      (UPernet.py:78-84): out (B*H*W, C) = hi (B*H*W, C) + up(lo (B*h*w, C)), the same weight rule, any h, w >= 1.
 *      out is another buffer than hi (hi == out: CMX_ERR_ARG): the BatchNorm + ReLU that produced hi still needs its
 *      own output in the backward.  The adjoint towards lo is cmx_upcat_multi_bwd with Cs = 0, n = 1. */
int cmx_up_add_fwd(const void* hi, const void* lo, void* out, int B, int h, int w, int H, int W, int C, int dtype, hipStream_t stream);

/* ---- Wf (C, KH*KW, N) contiguous, Wf[ci][KH*KW - 1 - t][co] = W[co][t][ci], from the tap-major 16-bit weights
 *      W (N, KH*KW, C) at row stride ldw elements (>= KH*KW*C, a multiple of 8); dtype 1 or 2 (0: CMX_ERR_DTYPE),
 *      N % 64 == 0, C % 8 == 0.  A tiled transpose through LDS, 16-byte accesses on both sides.  For a stride-1
 *      convolution with odd KH, KW and pad = (K - 1) / 2 the input gradient is then
 *      dx = cmx_conv_implicit_fwd(dy, Wf): fp32 accumulation over all taps and channels, rounded once. */
int cmx_conv_flip_weight(const void* W, void* Wf, int N, int KH, int KW, int C, int64_t ldw, int dtype, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif
