// Final upsample + plain CrossEntropyLoss, tiled through LDS (forward loss and fused backward).
//
// Same math as upsample_ce.hip (builder.py:233,249; train.py:72-73: bilinear x4 upsample,
// align_corners=False, then mean CE over pixels != ignore_index), re-tiled so that neither
// the full-resolution logits NOR their gradient ever reach HBM:
//  * forward: a block owns a 16 x 16 full-res tile, stages the low-res logits it reads
//    (<= 6 x 6 x K, fp32) in LDS once, and each thread does one pixel's interpolation +
//    log-softmax + NLL.  Only per-block loss / count partials are written.
//  * gradient: the cells kernel of loss_cells.h with the plain-CE criterion (LK_CE), the same
//    template loss_fused.hip instantiates for the loss family.  A block owns a CT_Y x CT_X
//    low-res tile of dlogits and recomputes the softmax gradient of every full-res pixel whose
//    bilinear footprint touches it, then applies the separable bilinear adjoint and writes the
//    tile once.  In training the forward runs it (FWD, with the loss partials) and the backward
//    only scales its fp32 result by dloss / n_valid; cmx_upsample_ce_bwd is the
//    recompute-in-backward form (FWD = false).  The 2-pass adjoint of a materialised
//    (B, H, W, K) gradient (49 MB at 480 x 640, K = 40) is gone.
#include "loss_cells.h"

namespace {

constexpr int FT = 16;                  // forward full-res tile edge
constexpr int LRF = FT / 4 + 3;         // low-res rows / cols a forward tile can read (scale <= 4)

// ------------------------------------------------------------------------ forward (loss only)
template <typename T>
__global__ __launch_bounds__(256) void ce_fwd_tiled(const T* __restrict__ logits, const int64_t* __restrict__ label,
                                                    float* __restrict__ part, int h, int w, int H, int W, int K,
                                                    int ignore, int tiles_x, int tiles_y) {
  __shared__ float lg[LRF * LRF * KF];
  __shared__ float red[2][256];
  const int bx = blockIdx.x % tiles_x, by = (blockIdx.x / tiles_x) % tiles_y, b = blockIdx.x / (tiles_x * tiles_y);
  const float sh = (float)h / H, sw = (float)w / W;
  const int Y0 = by * FT, X0 = bx * FT;
  int ly0, lx0, t1;
  float f0, f1;
  cmx_bilin_src(Y0, sh, h, ly0, t1, f0, f1);
  cmx_bilin_src(X0, sw, w, lx0, t1, f0, f1);
  const T* base = logits + (long)b * h * w * K;
  const int Y = Y0 + threadIdx.x / FT, X = X0 + threadIdx.x % FT;
  // every global load of the thread (its label, its share of the logits tile) is issued
  // before the first LDS store: one memory latency per block instead of one per 256 items
  const long lab = (Y < H && X < W) ? label[((long)b * H + Y) * W + X] : (long)ignore;
  constexpr int NL = (LRF * LRF * KF + 255) / 256;
  float v[NL];
#pragma unroll
  for (int i = 0; i < NL; ++i) {
    const int e = threadIdx.x + i * 256;
    const int k = e % K, px = e / K;
    const int yy = ly0 + px / LRF, xx = lx0 + px % LRF;
    v[i] = (e < LRF * LRF * K && yy < h && xx < w) ? to_f32(base[((long)yy * w + xx) * K + k]) : 0.f;
  }
#pragma unroll
  for (int i = 0; i < NL; ++i) {
    const int e = threadIdx.x + i * 256;
    if (e < LRF * LRF * K) lg[(e % K) * (LRF * LRF) + e / K] = v[i];   // class-major (see the backward)
  }
  __syncthreads();
  float ls = 0.f, lc = 0.f;
  if (Y < H && X < W) {
    if (!(lab == ignore || lab < 0 || lab >= K)) {
      int y0, y1, x0, x1;
      float wy0, wy1, wx0, wx1;
      cmx_bilin_src(Y, sh, h, y0, y1, wy0, wy1);
      cmx_bilin_src(X, sw, w, x0, x1, wx0, wx1);
      // class-major image [k][px] (49 pixels per class): the lanes of a wave read at most 10
      // distinct words per class, on distinct banks (a pixel-major [px][k] image put the wave's
      // low-res pixels 40 words apart: 1.7 bank conflicts per LDS read)
      constexpr int LP = LRF * LRF;
      const float* pa = lg + (y0 - ly0) * LRF + (x0 - lx0);
      const float* pb = lg + (y0 - ly0) * LRF + (x1 - lx0);
      const float* pc = lg + (y1 - ly0) * LRF + (x0 - lx0);
      const float* pd = lg + (y1 - ly0) * LRF + (x1 - lx0);
      // compile-time trip counts predicated on k < K: the LDS reads of all classes are in
      // flight together and z stays in registers (a runtime-bound loop waits on each read)
      float z[KF];
      float m = -INFINITY, zl = 0.f;
#pragma unroll
      for (int k = 0; k < KF; ++k) {
        z[k] = k < K ? wy0 * (wx0 * pa[k * LP] + wx1 * pb[k * LP]) + wy1 * (wx0 * pc[k * LP] + wx1 * pd[k * LP])
                     : -INFINITY;
        m = fmaxf(m, z[k]);
        if (k == lab) zl = z[k];
      }
      float se = 0.f;
#pragma unroll
      for (int k = 0; k < KF; ++k) se += __expf(z[k] - m);
      ls = m + __logf(se) - zl;
      lc = 1.f;
    }
  }
  red[0][threadIdx.x] = ls;
  red[1][threadIdx.x] = lc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      red[0][threadIdx.x] += red[0][threadIdx.x + o];
      red[1][threadIdx.x] += red[1][threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    part[blockIdx.x * 2] = red[0][0];
    part[blockIdx.x * 2 + 1] = red[1][0];
  }
}

// dlogits = adj * dloss[0] * stats[1]
template <typename T>
__global__ void ce_scale_kernel(const float* __restrict__ adj, const float* __restrict__ dloss,
                                const float* __restrict__ stats, T* __restrict__ dl, long n) {
  const float gs = dloss[0] * stats[1];
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    dl[i] = from_f32<T>(adj[i] * gs);
}

}  // namespace

// tiled forward (loss partials only); part: (B * tiles) x 2 floats
int ce_fwd_tiled_nblk(int B, int H, int W) { return B * ((H + FT - 1) / FT) * ((W + FT - 1) / FT); }

int ce_fwd_tiled_launch(const void* logits, const int64_t* label, float* part, int B, int h, int w, int H, int W,
                        int K, int ignore, int dtype, hipStream_t s) {
  const int tx = (W + FT - 1) / FT, ty = (H + FT - 1) / FT;
  CMX_DISPATCH(dtype, T, {
    hipLaunchKernelGGL(ce_fwd_tiled<T>, dim3(B * tx * ty), dim3(256), 0, s, (const T*)logits, label, part, h, w, H, W,
                       K, ignore, tx, ty);
  });
  return CMX_OK;
}

int ce_cells_fwd_launch(const void* logits, const int64_t* label, float* adj, float* part, int B, int h, int w, int H,
                        int W, int K, int ignore, int dtype, hipStream_t s) {
  CMX_DISPATCH(dtype, T, {
    loss_cells_launch<T, LK_CE, 0, true>((const T*)logits, label, nullptr, nullptr, nullptr, adj, part, B, h, w, H, W,
                                         K, ignore, 0.f, 0.f, 0.f, 0.f, s);
  });
  return cmx_check_launch("ce_cells_fwd");
}

extern "C" {

// dlogits (B, h, w, K) = bilinear-adjoint of (softmax - onehot) * dloss[0] * stats[1], with
// stats = cmx_upsample_ce_fwd's out ([loss, 1/n_valid, n_valid]).  H = 4h, W = 4w, K <= 40
// (every CMX dataset); otherwise use the grad output of cmx_upsample_ce_fwd and
// cmx_bilinear_adjoint_1d.
int cmx_upsample_ce_bwd(const void* logits, const int64_t* label, const float* dloss, const float* stats,
                        void* dlogits, int B, int h, int w, int H, int W, int K, int ignore_index, int dtype,
                        hipStream_t s) {
  CMX_REQUIRE(B > 0 && ce_tiled_ok(h, w, H, W, K), CMX_ERR_SHAPE,
              "upsample_ce_bwd: needs K <= %d and an exact x4 upsampling (K=%d, %dx%d -> %dx%d)", KF, K, h, w, H, W);
  CMX_DISPATCH(dtype, T, {
    loss_cells_launch<T, LK_CE, 0, false>((const T*)logits, label, nullptr, dloss, stats, dlogits, nullptr, B, h, w, H,
                                          W, K, ignore_index, 0.f, 0.f, 0.f, 0.f, s);
  });
  return cmx_check_launch("upsample_ce_bwd");
}

// the backward of cmx_upsample_ce_fwd_adj: dlogits = adj * dloss[0] * stats[1] (n elements)
int cmx_upsample_ce_bwd_scale(const float* adj, const float* dloss, const float* stats, void* dlogits, int64_t n,
                              int dtype, hipStream_t s) {
  CMX_REQUIRE(adj && dloss && stats && dlogits && n >= 0, CMX_ERR_ARG, "upsample_ce_bwd_scale: null operand");
  if (n == 0) return CMX_OK;
  const unsigned grid = (unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
  CMX_DISPATCH(dtype, T, {
    hipLaunchKernelGGL(ce_scale_kernel<T>, dim3(grid), dim3(256), 0, s, adj, dloss, stats, (T*)dlogits, (long)n);
  });
  return cmx_check_launch("upsample_ce_bwd_scale");
}

}  // extern "C"
