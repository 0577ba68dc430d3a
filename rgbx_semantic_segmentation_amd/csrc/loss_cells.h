// The cells kernel of the final upsample + loss: ONE kernel template with the criterion as a
// compile-time parameter, the finalize kernel, the tile constants, and the declarations the
// three translation units of the loss path share (ce_fused.hip: plain CE; loss_fused.hip: the
// family; upsample_ce.hip: the plain-CE entry points that launch into ce_fused.hip).
//
// With z = the x4 bilinear upsample (align_corners=False) of the low-res logits, p = softmax(z),
// y = the pixel's label, eps = 1e-8:
//   LK_CE   nn.CrossEntropyLoss()                 l = -log p_y                  norm = n_valid
//           (builder.py:233,249; train.py:72-73)  dl/dz_j = p_j - [j = y]
//   kind 0  nn.CrossEntropyLoss(weight=w)         l = w_y * -log p_y            norm = sum w_y
//           (train.py:72-73 with a class weight)  dl/dz_j = w_y (p_j - [j = y])
//   kind 1  FocalLoss2d (utils/loss_opr.py:12-23) l = -w_y (1 - p_y)^2 log p_y  norm = sum w_y
//           dl/dz_j = c (p_j - [j = y]),  c = w_y ((1 - p_y)^2 - 2 p_y (1 - p_y) log p_y)
//   kind 2  ce_scale * CE + focal_scale * FocalLoss (utils/loss_opr.py:158-202; CE_Focal,
//           builder.py:246-247, is (1, 0.2); pure FocalLoss is (0, 1))         norm = n_valid
//           focal l = -sum_k a_k x_k^gamma log(y_k + eps), (x, y, a)_k = (1 - p, p, alpha) at k = y,
//           (p, 1 - p, 1 - alpha) elsewhere; u_k = dl/dp_k; dl/dz_j = p_j (u_j - sum_k u_k p_k).
//           Labels are clamped to [0, K) and only label == ignore is invalid, as FocalLoss does.
// LK_CE and kinds 0 and 1 are the CE gradient times one scalar per pixel; kind 2 needs p_k of every
// class twice (sum_k u_k p_k, then the gradient): both passes recompute it from the run's two
// row-interpolated columns, as the kernel's own passes 2 and 3 do.
//
// DiceLoss / DiceCELoss (utils/loss_opr.py:103-156; dice_fused.hip) is not a per-pixel function: with
// v = (label != ignore), y = clamp(label, 0, K - 1) (FocalLoss's rule) and, per image b and class k,
// I = sum v p_k [y = k], P = sum v p_k, T = sum v [y = k], U = P + T over the image's pixels,
//   dice = (2 I + s) / (U + s),  DiceLoss = 1 - mean_(b,k) dice,
//   d DiceLoss / dp_k = u_k = v (c[b,k] - [y = k] a[b,k]),  c = (2 I + s) / ((U + s)^2 B K),
//   a = 2 / ((U + s) B K),  dl/dz_j = p_j (u_j - sum_k u_k p_k)  (kind 2's form).
// Two criteria of the template serve it:
//   LK_DSTAT  the statistics pass: per-block partials of I, P, T, the CE sum and the valid count over
//             the pixels the tile owns; ends after pass 2, no adjoint (t1 is never touched)
//   LK_DICE   the gradient pass, after dice_finalize_kernel made the coefficient table from the folded
//             statistics: dst = the adjoint of dL_dice/dz + cen (p - onehot), cen = ce_scale / n_valid;
//             the table (cw: per image c'[K], a'[K], cen; c', a' = dice_scale * c, a) is read from LDS
//
// ProbOhemCrossEntropy2d (utils/loss_opr.py:205-255; ohem_fused.hip) needs a global order statistic:
// with valid = (y != ignore and 0 <= y < K) (NLLLoss's rule) and p_y the valid pixels' target-class
// probability, kept = valid and p_y <= threshold, threshold = max(thresh, min_kept-th smallest p_y)
// (+inf when min_kept <= 0 or min_kept > n_valid: nothing is dropped), loss = mean over kept of -log p_y,
// dl/dz_j = (p_j - [j = y]) / n_kept at kept pixels, 0 elsewhere.  Two criteria of the template serve it:
//   LK_OSTAT  the statistics pass: py (B, H, W) fp32 = p_y of every pixel the tile owns (2.0 at a pixel
//             that is not valid) and the integer counts of the valid pixels and of those with
//             p_y <= thresh; ends after pass 2, no adjoint (t1 is never touched)
//   LK_OHEM   the gradient pass, after the select made the threshold: LK_CE's body with the pixels
//             whose stored py exceeds the device scalar threshold treated as ignored; no probability is
//             recomputed for the decision, so the two passes agree by construction
#pragma once
#include "cmx_common.h"

// ce_fused.hip, called from upsample_ce.hip.  Tiled loss-only forward; part: nblk x 2 floats
int ce_fwd_tiled_nblk(int B, int H, int W);
int ce_fwd_tiled_launch(const void* logits, const int64_t* label, float* part, int B, int h, int w, int H, int W,
                        int K, int ignore, int dtype, hipStream_t s);
// loss partials (part: loss_cells_nblk x 2 floats) and adj (B, h, w, K) fp32 = bilinear adjoint of
// (softmax - onehot), unscaled; exact x4, K <= 40
int ce_cells_fwd_launch(const void* logits, const int64_t* label, float* adj, float* part, int B, int h, int w, int H,
                        int W, int K, int ignore, int dtype, hipStream_t s);

namespace {   // kernels and constants: each including translation unit instantiates its own

constexpr int KF = 40;                  // classes held in LDS (NYUv2 40, Cityscapes 19, MFNet 9)
constexpr int CT_Y = 6, CT_X = 8;                 // low-res tile of a workgroup
constexpr int CT_R = 4 * CT_Y + 4;                // full-res footprint rows
constexpr int CT_C = CT_X + 1;                    // runs per footprint row
constexpr int CT_NT = 256;
static_assert(CT_R * CT_C <= CT_NT, "one run per thread");
constexpr float LOG2E = 1.4426950408889634f, LN2 = 0.69314718055994531f;
constexpr float FEPS = 1e-8f;

// LK_CE is internal: cmx_upsample_loss_fwd_adj's `kind` is 0..2
enum { LK_CE = -1, LK_WCE = 0, LK_FL2D = 1, LK_FOCAL = 2, LK_DICE = 3, LK_DSTAT = 4, LK_OHEM = 5, LK_OSTAT = 6 };
template <int LK> constexpr bool lk_dice = LK == LK_DICE || LK == LK_DSTAT;
template <int LK> constexpr bool lk_ce = LK == LK_CE || LK == LK_OHEM;   // the plain-CE body
constexpr float OHEM_SENTINEL = 2.f;    // py of a pixel that is not valid: above every probability
// gamma paths of kind 2: integer powers for 0, 1, 2, 4; GP_GEN = exp2(gamma * log2 x), gamma > 1
enum { GP_GEN = -1 };

// the tiles are sized for the decoder's exact x4 upsampling (MLPDecoder output at 1/4 res)
inline bool ce_tiled_ok(int h, int w, int H, int W, int K) { return K > 0 && K <= KF && H == 4 * h && W == 4 * w; }

inline int loss_cells_nblk(int B, int h, int w) { return B * ((h + CT_Y - 1) / CT_Y) * ((w + CT_X - 1) / CT_X); }
// Dice: floats per block of the statistics partials [I[K], P[K], T[K], CE sum, valid count], and per
// image of the coefficient table [c'[K], a'[K], cen]
__host__ __device__ constexpr int dice_part_stride(int K) { return 3 * K + 2; }
__host__ __device__ constexpr int dice_coef_stride(int K) { return 2 * K + 1; }

// x^(gamma - 1) and x^gamma for x in [0, 1]
template <int GP>
__device__ __forceinline__ void focal_pow(float x, float gamma, float& xg1, float& xg) {
  if constexpr (GP == 0) {
    xg1 = 0.f;                                    // only ever multiplied by gamma = 0
    xg = 1.f;
  } else if constexpr (GP == 1) {
    xg1 = 1.f;
    xg = x;
  } else if constexpr (GP == 2) {
    xg1 = x;
    xg = x * x;
  } else if constexpr (GP == 4) {
    const float x2 = x * x;
    xg1 = x2 * x;
    xg = x2 * x2;
  } else {
    xg1 = __builtin_amdgcn_exp2f((gamma - 1.f) * __builtin_amdgcn_logf(x));   // x = 0: exp2(-inf) = 0
    xg = xg1 * x;
  }
}

// one class of one pixel: e = exp2(z_k - shift), sv = sum_k e, inv = 1 / sv (0: invalid pixel),
// tgt = (k == y).  p, u = dl/dp_k, lt = the class's term of l.  1 - p is formed as (sv - e) / sv:
// no rounding of p enters it (sv >= e: sv is a sum of non-negative terms that include e).
template <int GP>
__device__ __forceinline__ void focal_class(float e, float sv, float inv, bool tgt, float gamma, float alpha,
                                            float& p, float& u, float& lt) {
  p = e * inv;
  const float q = fmaxf(sv - e, 0.f) * inv;
  const float x = tgt ? q : p, ye = (tgt ? p : q) + FEPS;
  const float as = tgt ? alpha : alpha - 1.f;     // u = as (gamma x^(gamma-1) log ye - x^gamma / ye)
  const float an = tgt ? -alpha : alpha - 1.f;    // lt = an x^gamma log ye
  const float L = __builtin_amdgcn_logf(ye) * LN2;
  const float r = __builtin_amdgcn_rcpf(ye);
  float xg1, xg;
  focal_pow<GP>(x, gamma, xg1, xg);
  if constexpr (GP == 0) u = -as * r;
  else u = as * __builtin_fmaf(gamma * xg1, L, -xg * r);
  lt = an * xg * L;
}

// -log p_y of one pixel (the target logit: 4 LDS reads at class offset q = y * LP)
__device__ __forceinline__ float target_nll(const float* la, const float* lb, int q, float wa2, float wb2, float cl,
                                            float cr, float shv, float sv) {
  const float zl = __builtin_fmaf(cl, __builtin_fmaf(wa2, la[q], wb2 * lb[q]),
                                  cr * __builtin_fmaf(wa2, la[q + 1], wb2 * lb[q + 1]));
  return (shv + __builtin_amdgcn_logf(sv) - zl) * LN2;
}

// Exact x4, align_corners=False: full-res X = 4x + r interpolates low-res columns (x - 1, x) for
// r = 0, 1 and (x, x + 1) for r = 2, 3, so the run X in [4c - 2, 4c + 2) reads columns c - 1 and
// c only (at the image borders the clamped taps put all weight on one of them) -- and, by the
// same weights, the adjoint of the x-interpolation sends the run's gradient to those two columns
// only.  A thread takes one such run of 4 pixels on one full-res row: 4 LDS reads per class give
// the run's two row-interpolated columns (registers, log2 units), from which the 4 pixels'
// logits, softmax and gradient follow; the softmax is shifted by the larger of the two columns'
// maxima (every pixel's logit is a convex combination of the two: an upper bound, no max pass),
// and the run's x-adjoint is its two column sums.  A workgroup owns a CT_Y x CT_X low-res tile
// of the output: the runs of full-res rows [4 y0 - 2, 4 y0 + 4 CT_Y + 2) and cells
// c = x0 .. x0 + CT_X (recompute (CT_X + 1) / CT_X x (CT_Y + 1) / CT_Y of the tile's own pixels);
// the column sums meet in LDS (the right column's first, the left column's added after a
// barrier: one fixed summation order), and the y-adjoint (8 full-res rows per low-res row)
// writes the tile.
//   FWD = true:  part[2 blk] = sum of l over the valid pixels the tile owns, part[2 blk + 1] =
//                their normaliser; dst (B, h, w, K) fp32 = the unscaled bilinear adjoint of dl/dz
//                (the backward only scales it: cmx_upsample_ce_bwd_scale)
//   FWD = false: LK_CE only, the recompute backward: dst in T = the adjoint of
//                (softmax - onehot) * dloss[0] * stats[1]
//   LK_DSTAT:    part[dice_part_stride(K) blk ..] = the block's statistics partials; dst unused
//   LK_DICE:     cw = the coefficient table; dst as FWD = true, final up to dloss; part unused
//   LK_OSTAT:    dst = py (B, H, W) fp32; part = two unsigned counters [n_valid, n_below], zeroed by the
//                caller, one integer atomic per block and counter; gamma = thresh
//   LK_OHEM:     cw = py, stats = the threshold (one float); dst and part as LK_CE with FWD = true, the
//                normaliser being the kept count
// cw, gamma, alpha, cs, fs: the criterion's parameters (see the top); LK_CE reads none of them.
template <typename T, int LK, int GP, bool FWD>
__global__ __launch_bounds__(CT_NT) void loss_cells(const T* __restrict__ logits, const int64_t* __restrict__ label,
                                                    const float* __restrict__ cw, const float* __restrict__ dloss,
                                                    const float* __restrict__ stats, void* __restrict__ dst,
                                                    float* __restrict__ part, int h, int w, int H, int W, int K,
                                                    int ignore, float gamma, float alpha, float cs, float fs,
                                                    int tiles_x, int tiles_y) {
  static_assert(FWD || LK == LK_CE, "the recompute backward exists for plain CE only");
  constexpr int LH = CT_Y + 2, LW = CT_X + 2, LP = LH * LW;   // low-res tile + 1-pixel halo
  constexpr int KP = KF + 1;                                   // odd pitch of the column sums
  __shared__ float lg[KF * LP];                                // class-major [k][row][col]
  __shared__ float t1[CT_R * CT_X * KP + KP];                  // x-adjoint [row][col][k] + a spare row
  __shared__ float wtab[CT_Y][8];                              // y-adjoint weights
  __shared__ float red[2][CT_NT / 64];
  const int t = threadIdx.x;
  const int bx = blockIdx.x % tiles_x, by = (blockIdx.x / tiles_x) % tiles_y, b = blockIdx.x / (tiles_x * tiles_y);
  const int y0 = by * CT_Y, x0 = bx * CT_X;
  const int ny = min(CT_Y, h - y0), nx = min(CT_X, w - x0);
  const float sh = (float)h / H, sw = (float)w / W;
  const int ri = t / CT_C, c = t % CT_C;          // the thread's run: footprint row, cell
  const bool act = ri < CT_R;
  const int Y = 4 * y0 - 2 + ri, X0 = 4 * (x0 + c) - 2;
  const bool rowin = act && Y >= 0 && Y < H;
  // global loads first: the run's labels, the thread's share of the logits tile -- all of them
  // unconditional (an out-of-range element reads the tile's first one and is replaced by a
  // select), so they are in flight together: a load under `cond ? load : 0` was sunk into its
  // branch and waited for there, 4 + NL round trips one after another
  long lab[4];
  bool labok[4];
  float pyv[4];                                   // LK_OHEM: the pixels' stored p_y
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int X = X0 + j;
    labok[j] = rowin && X >= 0 && X < W;
    lab[j] = label[labok[j] ? ((long)b * H + Y) * W + X : (long)b * H * W];
    if constexpr (LK == LK_OHEM) pyv[j] = cw[labok[j] ? ((long)b * H + Y) * W + X : (long)b * H * W];
  }
  float thr = 0.f;
  if constexpr (LK == LK_OHEM) thr = stats[0];
  const T* base = logits + (long)b * h * w * K;
  constexpr int NL = (LP * KF + CT_NT - 1) / CT_NT;
  float v[NL];
  bool vok[NL];
#pragma unroll
  for (int i = 0; i < NL; ++i) {
    const int e = t + i * CT_NT;
    const int k = e % K, px = e / K;                // coalesced along k
    const int yy = y0 - 1 + px / LW, xx = x0 - 1 + px % LW;
    vok[i] = e < LP * K && yy >= 0 && yy < h && xx >= 0 && xx < w;
    v[i] = to_f32(base[vok[i] ? ((long)yy * w + xx) * K + k : 0]);
  }
#pragma unroll
  for (int i = 0; i < NL; ++i) v[i] = vok[i] ? v[i] : 0.f;
  if (t < CT_Y * 8) {                             // low-res row y0 + yl from footprint row 4 yl + jj
    const int yl = t >> 3, r = 4 * yl + (t & 7);
    int ya, yb;
    float wa, wb;
    cmx_bilin_src(4 * y0 - 2 + r, sh, h, ya, yb, wa, wb);
    wtab[yl][t & 7] = (4 * y0 - 2 + r >= 0 && 4 * y0 - 2 + r < H)
                          ? (ya == y0 + yl ? wa : 0.f) + (yb == y0 + yl ? wb : 0.f) : 0.f;
  }
  int ya, yb;
  float wya, wyb;
  cmx_bilin_src(Y, sh, h, ya, yb, wya, wyb);      // rows outside the image: no valid pixel uses them
  // the 4 pixels' weights on the run's columns x0 + c - 1 (tile column c) and x0 + c (c + 1);
  // lv = the class of a valid pixel, -1 otherwise
  const int xl = x0 + c - 1, xr = x0 + c;
  float cl[4], cr[4];
  int lv[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    int i0, i1;
    float l0, l1;
    cmx_bilin_src(X0 + j, sw, w, i0, i1, l0, l1);
    cl[j] = (i0 == xl ? l0 : 0.f) + (i1 == xl ? l1 : 0.f);
    cr[j] = (i0 == xr ? l0 : 0.f) + (i1 == xr ? l1 : 0.f);
    if constexpr (LK == LK_FOCAL || lk_dice<LK>)  // FocalLoss: clamp(label, 0, K - 1), invalid only at ignore
      lv[j] = (labok[j] && lab[j] != ignore) ? (int)(lab[j] < 0 ? 0L : (lab[j] > K - 1 ? (long)(K - 1) : lab[j])) : -1;
    else if constexpr (LK == LK_OHEM)             // NLLLoss's rule and the select's: kept <=> py <= threshold
      lv[j] = (labok[j] && lab[j] >= 0 && lab[j] < K && lab[j] != ignore && pyv[j] <= thr) ? (int)lab[j] : -1;
    else                                          // NLLLoss
      lv[j] = (labok[j] && lab[j] >= 0 && lab[j] < K && lab[j] != ignore) ? (int)lab[j] : -1;
  }
  // class weights of the run's pixels (kinds 0, 1; NULL = 1): K floats, cached
  float wy[4];
  if constexpr (LK == LK_WCE || LK == LK_FL2D) {
#pragma unroll
    for (int j = 0; j < 4; ++j) wy[j] = cw != nullptr ? cw[lv[j] >= 0 ? lv[j] : 0] : 1.f;
  }
#pragma unroll
  for (int i = 0; i < NL; ++i) {
    const int e = t + i * CT_NT;
    if (e < LP * K) lg[(e % K) * LP + e / K] = v[i];
  }
  // classes K .. KF - 1: a very negative logit (exp2 -> 0 exactly, maxima unchanged), so the class
  // loops below run KF iterations without a test on K (a runtime test became a branch per class)
  for (int e = t; e < (KF - K) * LP; e += CT_NT) lg[K * LP + e] = -1e30f;
  // Dice: the image's coefficients c'[k] at ctab[k], a'[k] at ctab[KF + k] (padded classes 0), cen;
  // the statistics pass: the block's label counts and per-wave partial sums
  const float* ctab = nullptr;
  int* tcnt = nullptr;
  float (*wsum)[2 * KF + 2] = nullptr;
  float cen = 0.f;
  if constexpr (LK == LK_DICE) {
    __shared__ float ctab_s[2 * KF];
    const float* cb = cw + (long)b * dice_coef_stride(K);
    if (t < 2 * KF) ctab_s[t] = t % KF < K ? cb[(t / KF) * K + t % KF] : 0.f;
    cen = cb[2 * K];
    ctab = ctab_s;
  }
  if constexpr (LK == LK_DSTAT) {
    __shared__ int tcnt_s[KF];
    __shared__ float wsum_s[CT_NT / 64][2 * KF + 2];
    if (t < KF) tcnt_s[t] = 0;
    tcnt = tcnt_s;
    wsum = wsum_s;
  }
  unsigned* ocnt = nullptr;                       // LK_OSTAT: the block's [n_valid, n_below]
  if constexpr (LK == LK_OSTAT) {
    __shared__ unsigned ocnt_s[2];
    if (t < 2) ocnt_s[t] = 0;
    ocnt = ocnt_s;
  }
  __syncthreads();
  // pass 1: the run's two row-interpolated columns per class (registers, log2 units), the bound
  const float* la = lg + (min(max(ya - y0 + 1, 0), LH - 1)) * LW + c;
  const float* lb = lg + (min(max(yb - y0 + 1, 0), LH - 1)) * LW + c;
  const float wa2 = wya * LOG2E, wb2 = wyb * LOG2E;
  float ml[KF], mr[KF];
  float M = -INFINITY;
#pragma unroll
  for (int k = 0; k < KF; ++k) {
    ml[k] = __builtin_fmaf(wa2, la[k * LP], wb2 * lb[k * LP]);
    mr[k] = __builtin_fmaf(wa2, la[k * LP + 1], wb2 * lb[k * LP + 1]);
    M = fmaxf(M, fmaxf(ml[k], mr[k]));
  }
  // pass 2: the softmax denominators under the shared upper-bound shift (every exponent is <= 0;
  // pixels outside the image: shift 0, unused)
  float shv[4], sv[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    shv[j] = (cl[j] + cr[j]) * M;
    sv[j] = 0.f;
  }
#pragma unroll
  for (int k = 0; k < KF; ++k)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      sv[j] += __builtin_amdgcn_exp2f(__builtin_fmaf(cl[j], ml[k], __builtin_fmaf(cr[j], mr[k], -shv[j])));
  // a pixel whose own maximum lies more than ~100 binary orders below the bound (logits far apart
  // between neighbouring low-res pixels) underflowed: redo it with its own maximum (the focal terms
  // read 1 - p, so a flushed denominator would not do)
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (lv[j] >= 0 && !(sv[j] >= 0x1p-100f)) {
      float m = -INFINITY;
#pragma unroll
      for (int k = 0; k < KF; ++k) m = fmaxf(m, __builtin_fmaf(cl[j], ml[k], cr[j] * mr[k]));
      shv[j] = m;
      sv[j] = 0.f;
#pragma unroll
      for (int k = 0; k < KF; ++k)
        sv[j] += __builtin_amdgcn_exp2f(__builtin_fmaf(cl[j], ml[k], __builtin_fmaf(cr[j], mr[k], -m)));
    }
  if constexpr (LK == LK_OSTAT) {
    // p_y = e_y / sv of the pixels this tile owns, e_y formed exactly as class y's term of sv (so
    // p_y <= 1: sv is a sum of non-negative terms that include e_y); every pixel of the image is owned
    // by exactly one tile.  The counts are integers: order-independent
    float* py = reinterpret_cast<float*>(dst);
    const bool rown = Y >= 4 * y0 && Y < 4 * (y0 + CT_Y);
    unsigned nv = 0, nb = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int X = X0 + j;
      if (labok[j] && rown && X >= 4 * x0 && X < 4 * (x0 + CT_X)) {
        float p = OHEM_SENTINEL;
        if (lv[j] >= 0) {
          const int q = lv[j] * LP;
          const float mly = __builtin_fmaf(wa2, la[q], wb2 * lb[q]);
          const float mry = __builtin_fmaf(wa2, la[q + 1], wb2 * lb[q + 1]);
          p = __builtin_amdgcn_exp2f(__builtin_fmaf(cl[j], mly, __builtin_fmaf(cr[j], mry, -shv[j]))) / sv[j];
          nv += 1;
          nb += p <= gamma ? 1 : 0;
        }
        py[((long)b * H + Y) * W + X] = p;
      }
    }
    if (nv) atomicAdd(&ocnt[0], nv);
    if (nb) atomicAdd(&ocnt[1], nb);
    __syncthreads();
    if (t < 2 && ocnt[t]) atomicAdd(reinterpret_cast<unsigned*>(part) + t, ocnt[t]);
    return;
  }
  // gs: the scale of the whole gradient, a literal 1 in the forward.  The recompute backward folds
  // it into inv as gs / sv (not (1 / sv) * gs: the last bit differs)
  const float gs = FWD ? 1.f : dloss[0] * stats[1];
  float inv[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) inv[j] = lv[j] >= 0 ? gs / sv[j] : 0.f;
  if constexpr (LK == LK_DSTAT) {
    // the statistics of the valid pixels this tile owns.  Per class: the run's P and I terms summed
    // over the wave by the butterfly, the waves' sums met in LDS and added in wave order (no
    // floating-point atomic anywhere: one fixed order); the label counts are integers
    const bool rown = Y >= 4 * y0 && Y < 4 * (y0 + CT_Y);
    float ow[4], ls = 0.f, lc = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int X = X0 + j;
      const bool own = lv[j] >= 0 && rown && X >= 4 * x0 && X < 4 * (x0 + CT_X);
      ow[j] = own ? inv[j] : 0.f;
      if (own) {
        ls += target_nll(la, lb, lv[j] * LP, wa2, wb2, cl[j], cr[j], shv[j], sv[j]);
        lc += 1.f;
        atomicAdd(&tcnt[lv[j]], 1);
      }
    }
    const int wv = t >> 6;
    const bool lane0 = (t & 63) == 0;
#pragma unroll
    for (int k = 0; k < KF; ++k) {
      float pk = 0.f, ik = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float p = ow[j] * __builtin_amdgcn_exp2f(__builtin_fmaf(cl[j], ml[k], __builtin_fmaf(cr[j], mr[k], -shv[j])));
        pk += p;
        ik += k == lv[j] ? p : 0.f;
      }
      pk = wave_sum(pk);
      ik = wave_sum(ik);
      if (lane0) {
        wsum[wv][k] = ik;
        wsum[wv][KF + k] = pk;
      }
    }
    ls = wave_sum(ls);
    lc = wave_sum(lc);
    if (lane0) {
      wsum[wv][2 * KF] = ls;
      wsum[wv][2 * KF + 1] = lc;
    }
    __syncthreads();
    float* pb = part + (long)blockIdx.x * dice_part_stride(K);
    if (t < 2 * KF + 2) {
      float a = 0.f;
#pragma unroll
      for (int i = 0; i < CT_NT / 64; ++i) a += wsum[i][t];
      const int k = t % KF;
      if (t >= 2 * KF) pb[3 * K + t - 2 * KF] = a;
      else if (k < K) pb[(t / KF) * K + k] = a;
    } else if (t >= 128 && t < 128 + K) {
      pb[2 * K + t - 128] = (float)tcnt[t - 128];   // <= 768 pixels a tile: exact
    }
    return;
  }
  // per pixel: pl = its loss, pn = its share of the normaliser, pc = the factor on (p - onehot)
  float pl[4], pn[4], pc[4], S[4];
  if constexpr (lk_ce<LK>) {
    // pl is formed below, for the pixels the tile owns only (no other use of the target logit)
#pragma unroll
    for (int j = 0; j < 4; ++j) pc[j] = gs;
  } else if constexpr (LK == LK_DICE) {
    // pass 2b: sum_k u_k p_k, u_k = c'_k - [k = y] a'_k (a padded class and an invalid pixel: p = 0)
#pragma unroll
    for (int j = 0; j < 4; ++j) S[j] = 0.f;
#pragma unroll
    for (int k = 0; k < KF; ++k) {
      const float ck = ctab[k], ak = ctab[KF + k];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float e = __builtin_amdgcn_exp2f(__builtin_fmaf(cl[j], ml[k], __builtin_fmaf(cr[j], mr[k], -shv[j])));
        S[j] = __builtin_fmaf(e * inv[j], k == lv[j] ? ck - ak : ck, S[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      asm volatile("" : "+v"(S[j]));              // complete here, as kind 2's
      pc[j] = cen;
    }
  } else {
    // -log p_y of the valid pixels
    float nll[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      nll[j] = lv[j] >= 0 ? target_nll(la, lb, (lv[j] >= 0 ? lv[j] : 0) * LP, wa2, wb2, cl[j], cr[j], shv[j], sv[j])
                          : 0.f;
    if constexpr (LK == LK_WCE) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        pc[j] = wy[j];
        pl[j] = wy[j] * nll[j];
        pn[j] = wy[j];
      }
    } else if constexpr (LK == LK_FL2D) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float p = __builtin_amdgcn_exp2f(-nll[j] * LOG2E), om = 1.f - p, lp = -nll[j];
        pc[j] = wy[j] * om * __builtin_fmaf(-2.f * p, lp, om);
        pl[j] = -wy[j] * om * om * lp;
        pn[j] = wy[j];
      }
    } else {
      // pass 2b: sum_k u_k p_k and the focal loss, over the K real classes (a padded class has
      // p = 0 and contributes nothing for gamma >= 1; masked all the same: gamma = 0 leaves
      // -(1 - alpha) log(1 + eps) per class)
      float fl[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) S[j] = fl[j] = 0.f;
#pragma unroll
      for (int k = 0; k < KF; ++k) {
        const bool real = k < K;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float e = __builtin_amdgcn_exp2f(__builtin_fmaf(cl[j], ml[k], __builtin_fmaf(cr[j], mr[k], -shv[j])));
          float p, u, lt;
          focal_class<GP>(e, sv[j], inv[j], k == lv[j], gamma, alpha, p, u, lt);
          S[j] += real ? u * p : 0.f;
          fl[j] += real ? lt : 0.f;
        }
      }
      // the sums are complete HERE: left to itself the compiler sinks their per-class tails towards
      // their first use and keeps every class's operands live until then (scratch)
#pragma unroll
      for (int j = 0; j < 4; ++j) asm volatile("" : "+v"(S[j]), "+v"(fl[j]));
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        pc[j] = cs;
        pl[j] = __builtin_fmaf(fs, fl[j], cs * nll[j]);
        pn[j] = 1.f;
      }
    }
  }
  if constexpr (FWD && LK != LK_DICE) {
    // loss of the valid pixels this tile owns (full-res [4 y0, 4 y0 + 4 CT_Y) x [4 x0, 4 x0 + 4 CT_X))
    float ls = 0.f, lc = 0.f;
    const bool rown = Y >= 4 * y0 && Y < 4 * (y0 + CT_Y);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int X = X0 + j;
      const bool own = lv[j] >= 0 && rown && X >= 4 * x0 && X < 4 * (x0 + CT_X);
      if constexpr (lk_ce<LK>) {
        if (own) {
          ls += target_nll(la, lb, lv[j] * LP, wa2, wb2, cl[j], cr[j], shv[j], sv[j]);
          lc += 1.f;
        }
      } else {
        ls += own ? pl[j] : 0.f;
        lc += own ? pn[j] : 0.f;
      }
    }
    ls = wave_sum(ls);
    lc = wave_sum(lc);
    if ((t & 63) == 0) {
      red[0][t >> 6] = ls;
      red[1][t >> 6] = lc;
    }
  }
  // pass 3: the gradient's x-adjoint, the run's two column sums; the right column's go to LDS at
  // once (lanes with nothing to write write the spare row: no per-class branch), the left
  // column's wait in registers for the barrier; then the -onehot terms at the pixels' classes
  float* trow = t1 + (act ? ri : 0) * CT_X * KP;
  float* wrow = (act && c < CT_X) ? trow + c * KP : t1 + CT_R * CT_X * KP;
  float sl[KF];
  if constexpr (LK == LK_DICE) {
    // as kind 2's pass 3 below, with u from the table: g = p (u - S + cen)
#pragma unroll
    for (int j = 0; j < 4; ++j) asm volatile("" : "+v"(shv[j]), "+v"(lv[j]));
#pragma unroll
    for (int k = 0; k < KF; ++k) {
      const float ck = ctab[k], ak = ctab[KF + k];
      float gl = 0.f, gr = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float e = __builtin_amdgcn_exp2f(__builtin_fmaf(cl[j], ml[k], __builtin_fmaf(cr[j], mr[k], -shv[j])));
        const float g = e * inv[j] * ((k == lv[j] ? ck - ak : ck) - S[j] + cen);
        gl = __builtin_fmaf(cl[j], g, gl);
        gr = __builtin_fmaf(cr[j], g, gr);
      }
      wrow[k] = gr;
      sl[k] = gl;
    }
  } else if constexpr (LK == LK_FOCAL) {
    // the same exponentials and target selects as pass 2b, on purpose: opaque copies of the shifts
    // and classes keep the compiler from carrying pass 2b's per-class values (160 per thread and
    // kind) across to here instead (scratch)
#pragma unroll
    for (int j = 0; j < 4; ++j) asm volatile("" : "+v"(shv[j]), "+v"(lv[j]));
#pragma unroll
    for (int k = 0; k < KF; ++k) {
      float gl = 0.f, gr = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float e = __builtin_amdgcn_exp2f(__builtin_fmaf(cl[j], ml[k], __builtin_fmaf(cr[j], mr[k], -shv[j])));
        float p, u, lt;
        focal_class<GP>(e, sv[j], inv[j], k == lv[j], gamma, alpha, p, u, lt);
        const float g = p * __builtin_fmaf(fs, u - S[j], cs);   // invalid pixel, padded class: p = 0
        gl = __builtin_fmaf(cl[j], g, gl);
        gr = __builtin_fmaf(cr[j], g, gr);
      }
      wrow[k] = gr;                               // classes >= K: 0, never read
      sl[k] = gl;
    }
  } else {
    float al[4], ar[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if constexpr (lk_ce<LK>) {                  // inv carries gs already
        al[j] = cl[j] * inv[j];
        ar[j] = cr[j] * inv[j];
      } else {
        al[j] = cl[j] * inv[j] * pc[j];
        ar[j] = cr[j] * inv[j] * pc[j];
      }
    }
#pragma unroll
    for (int k = 0; k < KF; ++k) {
      float gl = 0.f, gr = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float e = __builtin_amdgcn_exp2f(__builtin_fmaf(cl[j], ml[k], __builtin_fmaf(cr[j], mr[k], -shv[j])));
        gl = __builtin_fmaf(al[j], e, gl);
        gr = __builtin_fmaf(ar[j], e, gr);
      }
      wrow[k] = gr;                               // classes >= K: 0, never read
      sl[k] = gl;
    }
  }
  if (act && c < CT_X)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (lv[j] >= 0) trow[c * KP + lv[j]] -= cr[j] * pc[j];
  __syncthreads();
  if (act && c >= 1) {
#pragma unroll
    for (int k = 0; k < KF; ++k) trow[(c - 1) * KP + k] += sl[k];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (lv[j] >= 0) trow[(c - 1) * KP + lv[j]] -= cl[j] * pc[j];
  }
  __syncthreads();
  if constexpr (FWD && LK != LK_DICE) {
    if (t == 0) {
      float a = 0.f, n = 0.f;
#pragma unroll
      for (int i = 0; i < CT_NT / 64; ++i) {
        a += red[0][i];
        n += red[1][i];
      }
      part[blockIdx.x * 2] = a;
      part[blockIdx.x * 2 + 1] = n;
    }
  }
  // y-adjoint: low-res row y takes full-res rows [4y - 2, 4y + 6) = footprint rows [4 yl, 4 yl + 8)
  for (int e = t; e < CT_Y * CT_X * KF; e += CT_NT) {
    const int k = e % KF, xq = (e / KF) % CT_X, yl = e / (KF * CT_X);
    if (k >= K || xq >= nx || yl >= ny) continue;
    const float* tc = t1 + (4 * yl * CT_X + xq) * KP + k;
    float acc = 0.f;
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) acc = __builtin_fmaf(wtab[yl][jj], tc[jj * CT_X * KP], acc);
    const long o = ((long)b * h * w + (long)(y0 + yl) * w + x0 + xq) * K + k;
    if constexpr (FWD) reinterpret_cast<float*>(dst)[o] = acc;
    else reinterpret_cast<T*>(dst)[o] = from_f32<T>(acc);
  }
}

// grid for B x h x w low-res pixels; the arguments a criterion does not read may be NULL / 0
template <typename T, int LK, int GP, bool FWD>
void loss_cells_launch(const T* logits, const int64_t* label, const float* cw, const float* dloss, const float* stats,
                       void* dst, float* part, int B, int h, int w, int H, int W, int K, int ignore, float gamma,
                       float alpha, float cs, float fs, hipStream_t s) {
  const int tx = (w + CT_X - 1) / CT_X, ty = (h + CT_Y - 1) / CT_Y;
  hipLaunchKernelGGL((loss_cells<T, LK, GP, FWD>), dim3(B * tx * ty), dim3(CT_NT), 0, s, logits, label, cw, dloss,
                     stats, dst, part, h, w, H, W, K, ignore, gamma, alpha, cs, fs, tx, ty);
}

// out[0] = loss = sum / norm, out[1] = 1 / norm, out[2] = norm.  ZERO_EMPTY (pure FocalLoss):
// norm + eps in the quotients and loss 0 when nothing is valid; otherwise torch's mean (NaN then).
template <bool ZERO_EMPTY>
__global__ void loss_finalize_kernel(const float* __restrict__ part, int nblk, float* __restrict__ out) {
  __shared__ double red[2][256];
  double s = 0.0, c = 0.0;
  for (int i = threadIdx.x; i < nblk; i += 256) { s += part[2 * i]; c += part[2 * i + 1]; }
  red[0][threadIdx.x] = s;
  red[1][threadIdx.x] = c;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) { red[0][threadIdx.x] += red[0][threadIdx.x + o]; red[1][threadIdx.x] += red[1][threadIdx.x + o]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double cnt = red[1][0];
    if constexpr (ZERO_EMPTY) {
      out[0] = cnt > 0 ? (float)(red[0][0] / (cnt + 1e-8)) : 0.f;
      out[1] = cnt > 0 ? (float)(1.0 / (cnt + 1e-8)) : 0.f;
    } else {
      out[0] = cnt > 0 ? (float)(red[0][0] / cnt) : NAN;   // PyTorch: mean over zero valid pixels is NaN
      out[1] = cnt > 0 ? (float)(1.0 / cnt) : 0.f;
    }
    out[2] = (float)cnt;
  }
}

}  // namespace
