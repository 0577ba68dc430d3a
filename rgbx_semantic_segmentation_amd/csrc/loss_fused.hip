// Final upsample + the loss family beside plain CrossEntropyLoss: the cells kernel of
// loss_cells.h (where the criteria are stated) instantiated for kinds 0..2, the same template
// ce_fused.hip instantiates for plain CE.  Forward: loss partials + the unscaled fp32 bilinear
// adjoint of the per-pixel gradient at low resolution, in ONE pass over the full-resolution
// pixels; the backward is cmx_upsample_ce_bwd_scale.  No full-resolution tensor is ever
// materialised.
#include "loss_cells.h"

extern "C" {

size_t cmx_upsample_loss_workspace(int B, int h, int w) {
  if (B <= 0 || h <= 0 || w <= 0) return 0;
  return (size_t)loss_cells_nblk(B, h, w) * 2 * sizeof(float);
}

int cmx_upsample_loss_fwd_adj(const void* logits, const int64_t* label, const float* class_weight, float* adj,
                              float* out, float* workspace, int B, int h, int w, int H, int W, int K,
                              int ignore_index, int kind, float gamma, float alpha, float ce_scale, float focal_scale,
                              int dtype, hipStream_t s) {
  CMX_REQUIRE(B > 0 && h > 0 && w > 0 && ce_tiled_ok(h, w, H, W, K), CMX_ERR_SHAPE,
              "upsample_loss_fwd_adj: needs H = 4h, W = 4w, K <= %d (K=%d, %dx%d -> %dx%d)", KF, K, h, w, H, W);
  CMX_REQUIRE(kind >= LK_WCE && kind <= LK_FOCAL, CMX_ERR_ARG,
              "upsample_loss_fwd_adj: kind %d (0 weighted CE, 1 FocalLoss2d, 2 ce_scale CE + focal_scale FocalLoss)",
              kind);
  CMX_REQUIRE(kind != LK_FOCAL || ((gamma == 0.f || gamma >= 1.f) && !class_weight), CMX_ERR_ARG,
              "upsample_loss_fwd_adj: FocalLoss takes gamma == 0 or gamma >= 1 (%g) and no class weight", (double)gamma);
  CMX_REQUIRE(logits && label && adj && out && workspace, CMX_ERR_ARG, "upsample_loss_fwd_adj: null operand");
  const int nb = loss_cells_nblk(B, h, w);
#define CMX_LOSS_LAUNCH(LK, GP)                                                                                       \
  CMX_DISPATCH(dtype, T, {                                                                                            \
    loss_cells_launch<T, LK, GP, true>((const T*)logits, label, class_weight, nullptr, nullptr, adj, workspace, B, h, \
                                       w, H, W, K, ignore_index, gamma, alpha, ce_scale, focal_scale, s);             \
  })
  if (kind == LK_WCE) CMX_LOSS_LAUNCH(LK_WCE, 0);
  else if (kind == LK_FL2D) CMX_LOSS_LAUNCH(LK_FL2D, 0);
  else if (gamma == 0.f) CMX_LOSS_LAUNCH(LK_FOCAL, 0);
  else if (gamma == 1.f) CMX_LOSS_LAUNCH(LK_FOCAL, 1);
  else if (gamma == 2.f) CMX_LOSS_LAUNCH(LK_FOCAL, 2);
  else if (gamma == 4.f) CMX_LOSS_LAUNCH(LK_FOCAL, 4);
  else CMX_LOSS_LAUNCH(LK_FOCAL, GP_GEN);
#undef CMX_LOSS_LAUNCH
  if (kind == LK_FOCAL && ce_scale == 0.f)
    hipLaunchKernelGGL(loss_finalize_kernel<true>, dim3(1), dim3(256), 0, s, workspace, nb, out);
  else
    hipLaunchKernelGGL(loss_finalize_kernel<false>, dim3(1), dim3(256), 0, s, workspace, nb, out);
  return cmx_check_launch("upsample_loss_fwd_adj");
}

}  // extern "C"
