// Final upsample + DiceLoss / DiceCELoss (utils/loss_opr.py:103-156; the math is stated at the top
// of loss_cells.h).  Dice needs per-image, per-class sums over all pixels before any gradient can be
// formed, so the forward is three launches, none of which materialises a full-resolution tensor:
//   1. loss_cells<LK_DSTAT>: per-block partials of I, P, T, the CE sum and the valid count
//   2. dice_finalize_kernel: the partials folded per (image, class) in fp64 in a fixed order ->
//      stats, the coefficient table, out = [loss, backward factor, n_valid] (the loss is complete)
//   3. loss_cells<LK_DICE>: adj = the bilinear adjoint of dice_scale dL_dice/dz + ce_scale
//      (p - onehot) / n_valid, final up to dloss; not launched when adj is NULL (loss only)
// The backward is cmx_upsample_ce_bwd_scale with out[1] = 1.  No floating-point atomic is used:
// every result is bit-identical from run to run.
#include "loss_cells.h"

namespace {

constexpr int DF_NT = 1024;             // threads of the finalize block
constexpr int DF_Q = 128;               // columns of a partial row, padded (3 KF + 2 <= 128)
constexpr int DF_G = DF_NT / DF_Q;      // row groups
constexpr int DF_U = 8;                 // rows a thread loads per round
static_assert(3 * KF + 2 <= DF_Q, "a partial row fits the column groups");

// One block.  Image by image: group g of the threads sums rows g, g + DF_G, ... of the image's
// `tiles` partial rows per column in fp64, the groups' sums are added in group order, then thread k
// forms class k's dice and coefficients.  stats (B, K, 3) = I, P, T; coef (B, 2K + 1) = c', a', cen.
__global__ __launch_bounds__(DF_NT) void dice_finalize_kernel(const float* __restrict__ part, int tiles, int B, int K,
                                                              float cs, float ds, float smooth,
                                                              float* __restrict__ stats, float* __restrict__ coef,
                                                              float* __restrict__ out) {
  __shared__ double acc[DF_G][DF_Q];
  __shared__ double dsum[KF];
  const int t = threadIdx.x, q = t % DF_Q, g = t / DF_Q;
  const int Q = dice_part_stride(K), CS = dice_coef_stride(K);
  const double s = smooth, bk = (double)B * K;
  double dk = 0.0, ce = 0.0, nv = 0.0;  // thread k: sum over the images of dice[., k]; thread 0: CE sum, n_valid
  for (int b = 0; b < B; ++b) {
    // DF_U rows of the group per round, their loads in flight together (one block folds everything:
    // the time is load latency), into DF_U accumulators added in a fixed order
    double au[DF_U] = {};
    if (q < Q) {
      const float* pq = part + (long)b * tiles * Q + q;
      int i = g;
      for (; i + (DF_U - 1) * DF_G < tiles; i += DF_U * DF_G) {
        float f[DF_U];
#pragma unroll
        for (int u = 0; u < DF_U; ++u) f[u] = pq[(long)(i + u * DF_G) * Q];
#pragma unroll
        for (int u = 0; u < DF_U; ++u) au[u] += f[u];
      }
      for (; i < tiles; i += DF_G) au[0] += pq[(long)i * Q];
    }
    double a = 0.0;
#pragma unroll
    for (int u = 0; u < DF_U; ++u) a += au[u];
    acc[g][q] = a;
    __syncthreads();
    if (t < Q) {
      double f = 0.0;
#pragma unroll
      for (int i = 0; i < DF_G; ++i) f += acc[i][t];
      acc[0][t] = f;                    // column t is this thread's alone
    }
    __syncthreads();
    if (t < K) {
      const double I = acc[0][t], P = acc[0][K + t], T = acc[0][2 * K + t], U = P + T;
      dk += (2.0 * I + s) / (U + s);
      float* st = stats + ((long)b * K + t) * 3;
      st[0] = (float)I;
      st[1] = (float)P;
      st[2] = (float)T;
      coef[(long)b * CS + t] = (float)(ds * (2.0 * I + s) / ((U + s) * (U + s) * bk));
      coef[(long)b * CS + K + t] = (float)(ds * 2.0 / ((U + s) * bk));
    }
    if (t == 0) {
      ce += acc[0][3 * K];
      nv += acc[0][3 * K + 1];
    }
    __syncthreads();
  }
  if (t < K) dsum[t] = dk;
  __syncthreads();
  if (t == 0) {
    double d = 0.0;
    for (int k = 0; k < K; ++k) d += dsum[k];
    // nothing valid: every dice is s / s = 1 and the Dice term is exactly 0; the CE term is torch's
    // mean (NaN), and the backward factor 0 then keeps the gradient zero
    double loss = ds * (1.0 - d / bk);
    if (cs != 0.f) loss += nv > 0 ? cs * ce / nv : (double)NAN;
    out[0] = (float)loss;
    out[1] = (cs != 0.f && !(nv > 0)) ? 0.f : 1.f;
    out[2] = (float)nv;
    const float cen = (cs != 0.f && nv > 0) ? (float)(cs / nv) : 0.f;
    for (int b = 0; b < B; ++b) coef[(long)b * CS + 2 * K] = cen;
  }
}

}  // namespace

extern "C" {

size_t cmx_upsample_dice_workspace(int B, int h, int w, int K) {
  if (B <= 0 || h <= 0 || w <= 0 || K <= 0 || K > KF) return 0;
  return ((size_t)loss_cells_nblk(B, h, w) * dice_part_stride(K) + (size_t)B * dice_coef_stride(K)) * sizeof(float);
}

int cmx_upsample_dice_fwd_adj(const void* logits, const int64_t* label, float* adj, float* out, float* stats,
                              float* workspace, int B, int h, int w, int H, int W, int K, int ignore_index,
                              float ce_scale, float dice_scale, float smooth, int dtype, hipStream_t s) {
  CMX_REQUIRE(B > 0 && h > 0 && w > 0 && ce_tiled_ok(h, w, H, W, K), CMX_ERR_SHAPE,
              "upsample_dice_fwd_adj: needs H = 4h, W = 4w, K <= %d (K=%d, %dx%d -> %dx%d)", KF, K, h, w, H, W);
  CMX_REQUIRE(smooth > 0.f && ce_scale >= 0.f && dice_scale >= 0.f, CMX_ERR_ARG,
              "upsample_dice_fwd_adj: needs smooth > 0 (%g) and ce_scale, dice_scale >= 0 (%g, %g)", (double)smooth,
              (double)ce_scale, (double)dice_scale);
  CMX_REQUIRE(dtype >= 0 && dtype <= 2, CMX_ERR_DTYPE, "upsample_dice_fwd_adj: unsupported dtype %d", dtype);
  CMX_REQUIRE(logits && label && out && stats && workspace, CMX_ERR_ARG, "upsample_dice_fwd_adj: null operand");
  const int nb = loss_cells_nblk(B, h, w);
  float* part = workspace;
  float* coef = workspace + (size_t)nb * dice_part_stride(K);
  CMX_DISPATCH(dtype, T, {
    loss_cells_launch<T, LK_DSTAT, 0, true>((const T*)logits, label, nullptr, nullptr, nullptr, nullptr, part, B, h, w,
                                            H, W, K, ignore_index, 0.f, 0.f, 0.f, 0.f, s);
  });
  hipLaunchKernelGGL(dice_finalize_kernel, dim3(1), dim3(DF_NT), 0, s, part, nb / B, B, K, ce_scale, dice_scale,
                     smooth, stats, coef, out);
  if (adj)
    CMX_DISPATCH(dtype, T, {
      loss_cells_launch<T, LK_DICE, 0, true>((const T*)logits, label, coef, nullptr, nullptr, adj, nullptr, B, h, w, H,
                                             W, K, ignore_index, 0.f, 0.f, 0.f, 0.f, s);
    });
  return cmx_check_launch("upsample_dice_fwd_adj");
}

}  // extern "C"
