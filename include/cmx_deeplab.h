/* cmx_deeplab.h — C-ABI of libcmx_hip.so, part 5: what the DeepLabV3+ decode head (models/decoders/deeplabv3plus.py)
 * needs beyond the GEMM family and the eASPP neck's kernels: ASPP's wide dilated 3x3 convolutions on one shared input,
 * and the align_corners=True upsample + concat of the decoder.  The conventions, the status codes, CMX_ABI_VERSION and
 * hipStream_t are cmx_hip.h's; the Python binding parses this file as it parses that one (every declaration on one
 * line) and keeps its entry points in a table of their own (_lib.DEEPLAB_SIGNATURES).
 */
#ifndef CMX_DEEPLAB_H
#define CMX_DEEPLAB_H
#include "cmx_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- grouped dilated 3x3 convolution Cin -> Cout, stride 1, dilation = padding = rate, no bias (ASPP.b1 .. b3,
 *      deeplabv3plus.py:37-47): ONE launch runs the three branches, which all read the SAME input x.  Cin and Cout
 *      are multiples of 64, at most 1024 (anything else: CMX_ERR_SHAPE).  Activations are token-major NHWC rows
 *      (B*h*w of them) with a row stride in elements (>= the row's channels, a multiple of 16 bytes; bases 16-byte
 *      aligned); weights are the flat store's tap-major (Cout, kh, kw, Cin), contiguous.  fp32 accumulation on MFMA
 *      for all three dtypes (fp32: the exact 32x32x2 form).  Zero padding and tap skipping as cmx_easpp_conv_*: a tap
 *      whose offset (ky - 1, kx - 1) * rate leaves the map for EVERY pixel (|dy| >= h or |dx| >= w) is skipped as a
 *      whole, which is exact.  No im2col buffer.
 *      fwd:   y_g[p][co] = sum_tap sum_ci x[p + off_g(tap)][ci] * w_g[co][tap][ci], g = 0..2
 *      dgrad: dx[p][ci]  = sum_g sum_tap sum_co dy_g[p - off_g(tap)][co] * w_g[co][tap][ci]: the SUM over the three
 *             branches, accumulated in fp32 and rounded once (the three dy_g share lddy).
 *      wgrad: dw_g[co][tap][ci] = sum_p dy_g[p][co] * x[p + off_g(tap)][ci], fp32, OVERWRITTEN (a skipped tap is
 *             written as zeros).  One wave per (row chunk, tap, branch, 64 x 64 slice); the rows are split into at
 *             most 8 chunks of at least 128 * min(16, Cin/64 * Cout/64) rows.  With more than one chunk the per-chunk
 *             partials go to `workspace` (cmx_aspp_conv_wgrad_workspace bytes; 0 for one chunk and for a shape the
 *             entry point refuses) and a second launch folds them in chunk order: no float atomics, bit-identical
 *             from run to run.
 *      A NULL operand, a rate < 1, a misaligned base or stride: CMX_ERR_ARG; B, h, w <= 0 or a channel count that is
 *      no multiple of 64 in 64..1024: CMX_ERR_SHAPE; an unknown dtype: CMX_ERR_DTYPE. */
int cmx_aspp_conv_fwd(const void* x, const void* w0, const void* w1, const void* w2, void* y0, void* y1, void* y2, int B, int h, int w, int Cin, int Cout, int r0, int r1, int r2, int64_t ldx, int64_t ldy, int dtype, hipStream_t stream);
int cmx_aspp_conv_dgrad(const void* dy0, const void* dy1, const void* dy2, const void* w0, const void* w1, const void* w2, void* dx, int B, int h, int w, int Cin, int Cout, int r0, int r1, int r2, int64_t lddy, int64_t lddx, int dtype, hipStream_t stream);
size_t cmx_aspp_conv_wgrad_workspace(int B, int h, int w, int Cin, int Cout);
int cmx_aspp_conv_wgrad(const void* dy0, const void* dy1, const void* dy2, const void* x, float* dw0, float* dw1, float* dw2, float* workspace, int B, int h, int w, int Cin, int Cout, int r0, int r1, int r2, int64_t lddy, int64_t ldx, int dtype, hipStream_t stream);

/* ---- F.interpolate(lo, (H, W), mode='bilinear', align_corners=True) + torch.cat([., skip], 1) (deeplabv3plus.py:32-33)
 *      in one launch: cat (B*H*W, C + Cs) = [up_ac(lo) | skip], lo (B*h*w, C), skip (B*H*W, Cs), all contiguous in the
 *      storage dtype with 16-byte aligned bases; any 1 <= h <= H, 1 <= w <= W; C % 64 == 0, Cs % 8 == 0, Cs > 0.
 *      torch's align_corners=True rule in fp32: scale = (h - 1) / (H - 1) if H > 1 else 0, src = scale * Y,
 *      y0 = min(floor(src), h - 1), y1 = min(y0 + 1, h - 1), lambda = src - y0; columns likewise.
 *      bwd, one launch: dskip = dcat's columns [C, C + Cs); dlo[b][r][c][:] = sum_Y sum_X wy(Y, r) wx(X, c)
 *      dcat[b][Y][X][:C] as a gather over the output pixels whose taps touch (r, c), with the forward's own indices
 *      and weights, in fp32, rows dealt to four waves whose sums are added in a fixed order: no atomics,
 *      bit-identical from run to run, no workspace.
 *      A NULL operand or a base off a 16-byte boundary: CMX_ERR_ARG; a shape outside the above: CMX_ERR_SHAPE. */
int cmx_upcat_ac_fwd(const void* lo, const void* skip, void* cat, int B, int h, int w, int H, int W, int C, int Cs, int dtype, hipStream_t stream);
int cmx_upcat_ac_bwd(const void* dcat, void* dlo, void* dskip, int B, int h, int w, int H, int W, int C, int Cs, int dtype, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif
