// Final upsample + loss at the scales of an FCN head: bilinear x S (align_corners=False), S in {8, 16, 32},
// fused with plain CE and kinds 0..2 of loss_cells.h (the criteria are stated there; the per-class helpers,
// the constants and the finalize kernel are its own).  The x4 cells kernel is not touched.
//
// Runs of S.  With scale 1 / S (exact in fp32) full-res X = S c + r reads low-res columns (c - 1, c) for
// r < S / 2 and (c, c + 1) otherwise: the S columns [S c - S/2, S c + S/2) read columns c - 1 and c only,
// every weight a multiple of 1 / (2S); rows likewise.  So the S x S pixels of cell (r, c), r in [0, h],
// c in [0, w] (clipped at the image: the border cells are half cells whose clamped taps put all weight on
// one row / column), depend on the four low-res pixels (r - 1 .. r, c - 1 .. c) alone, and the adjoint of
// their gradient lands on those four.  Every full-res pixel lies in exactly one cell.
//
// A thread takes 4 pixels of one cell row, as loss_cells' thread takes its run of 4: 4 LDS reads per class
// give the row-interpolated left and right columns (registers, log2 units), the softmax is shifted by the
// larger of the two columns' maxima, and the gradient's x-adjoint is two sums per class.  The S / 4 threads
// of a cell row add theirs by a DPP butterfly (one fixed order); the rows meet in LDS, and the y-adjoint
// adds a cell's S rows per class and corner in row order.  A workgroup of 256 threads holds 1024 / S^2 cells
// of one cell row (16, 4, 1): their two low-res rows and one column of halo are staged in LDS.
// Per cell the four corner sums go to the workspace, (B, h + 1, w + 1, 4, KF) fp32: a gather kernel then adds
// each low-res pixel's four (one per adjacent cell) in a fixed order into adj.  No full-resolution tensor is
// written, the labels are read once, and no floating-point atomic is used.
#include "loss_cells.h"
#include "../../include/cmx_fcn.h"

namespace {

constexpr int SC_NT = 256;
constexpr int SC_LW = 17;                         // staged columns: up to 16 cells + 1
constexpr int SC_LP = 2 * SC_LW;                  // class pitch: two low-res rows
constexpr int SC_ROWS = 128;                      // cell rows of a workgroup: 1024 / S <= 128
constexpr int SC_KP = KF + 1;

inline bool scaled_ok(int S) { return S == 8 || S == 16 || S == 32; }
inline int scaled_cpw(int S) { return 1024 / (S * S); }                     // cells per workgroup
inline int scaled_groups_x(int w, int S) { return (w + 1 + scaled_cpw(S) - 1) / scaled_cpw(S); }
inline long scaled_nblk(int B, int h, int w, int S) { return (long)B * (h + 1) * scaled_groups_x(w, S); }

// cell: the corner sums, [b][r][c][q][KF], q = 2 * (bottom row r) + (right column c)
template <typename T, int LK, int GP>
__global__ __launch_bounds__(SC_NT) void loss_scaled_cells(const T* __restrict__ logits,
                                                           const int64_t* __restrict__ label,
                                                           const float* __restrict__ cw, float* __restrict__ cell,
                                                           float* __restrict__ part, int h, int w, int S, int K,
                                                           int ignore, float gamma, float alpha, float cs, float fs,
                                                           int groups_x) {
  constexpr int LP = SC_LP;
  __shared__ float lg[KF * SC_LP];                // class-major [k][row][col]
  __shared__ float t1[SC_ROWS * 2 * SC_KP];       // x-adjoint [cell row][left | right][k]
  __shared__ float wrow[SC_ROWS][2];              // y-adjoint weights [cell row][top | bottom]
  __shared__ float red[2][SC_NT / 64];
  const int t = threadIdx.x;
  const int SEG = S >> 2, TPC = S * SEG, CPW = SC_NT / TPC;
  const int gx = blockIdx.x % groups_x, r = (blockIdx.x / groups_x) % (h + 1), b = blockIdx.x / (groups_x * (h + 1));
  const int c0 = gx * CPW;
  const int H = S * h, W = S * w;
  const float sh = 1.f / (float)S;                // (float)h / H, exact
  const int cc = t / TPC, ri = (t % TPC) / SEG, seg = t % SEG, rowi = t / SEG;
  const int c = c0 + cc;
  const int Y = S * r - (S >> 1) + ri, X0 = S * c - (S >> 1) + 4 * seg;
  const bool rowin = c <= w && Y >= 0 && Y < H;
  // global loads first, all unconditional (loss_cells.h: an out-of-range element reads a valid address and is
  // replaced by a select)
  long lab[4];
  bool labok[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int X = X0 + j;
    labok[j] = rowin && X >= 0 && X < W;
    lab[j] = label[labok[j] ? ((long)b * H + Y) * W + X : (long)b * H * W];
  }
  const T* base = logits + (long)b * h * w * K;
  constexpr int NL = (SC_LP * KF + SC_NT - 1) / SC_NT;
  float v[NL];
  bool vok[NL];
#pragma unroll
  for (int i = 0; i < NL; ++i) {
    const int e = t + i * SC_NT;
    const int k = e % K, px = e / K;                // coalesced along k
    const int yy = r - 1 + px / SC_LW, xx = c0 - 1 + px % SC_LW;
    vok[i] = e < LP * K && yy >= 0 && yy < h && xx >= 0 && xx < w;
    v[i] = to_f32(base[vok[i] ? ((long)yy * w + xx) * K + k : 0]);
  }
#pragma unroll
  for (int i = 0; i < NL; ++i) v[i] = vok[i] ? v[i] : 0.f;
  // the row's weights on low-res rows r - 1 (top) and r (bottom); a row outside the image: 0, 0
  int ya, yb;
  float wya, wyb;
  cmx_bilin_src(Y, sh, h, ya, yb, wya, wyb);
  const float wtop = (ya == r - 1 ? wya : 0.f) + (yb == r - 1 ? wyb : 0.f);
  const float wbot = (ya == r ? wya : 0.f) + (yb == r ? wyb : 0.f);
  if (seg == 0) {
    wrow[rowi][0] = rowin ? wtop : 0.f;
    wrow[rowi][1] = rowin ? wbot : 0.f;
  }
  // the 4 pixels' weights on columns c - 1 (staged column cc) and c (cc + 1); lv = the class of a valid pixel
  float cl[4], cr[4];
  int lv[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    int i0, i1;
    float l0, l1;
    cmx_bilin_src(X0 + j, sh, w, i0, i1, l0, l1);
    cl[j] = (i0 == c - 1 ? l0 : 0.f) + (i1 == c - 1 ? l1 : 0.f);
    cr[j] = (i0 == c ? l0 : 0.f) + (i1 == c ? l1 : 0.f);
    if constexpr (LK == LK_FOCAL)                 // FocalLoss: clamp(label, 0, K - 1), invalid only at ignore
      lv[j] = (labok[j] && lab[j] != ignore) ? (int)(lab[j] < 0 ? 0L : (lab[j] > K - 1 ? (long)(K - 1) : lab[j])) : -1;
    else                                          // NLLLoss
      lv[j] = (labok[j] && lab[j] >= 0 && lab[j] < K && lab[j] != ignore) ? (int)lab[j] : -1;
  }
  float wy[4];
  if constexpr (LK == LK_WCE || LK == LK_FL2D) {
#pragma unroll
    for (int j = 0; j < 4; ++j) wy[j] = cw != nullptr ? cw[lv[j] >= 0 ? lv[j] : 0] : 1.f;
  }
#pragma unroll
  for (int i = 0; i < NL; ++i) {
    const int e = t + i * SC_NT;
    if (e < LP * K) lg[(e % K) * LP + e / K] = v[i];
  }
  // classes K .. KF - 1: a very negative logit (exp2 -> 0 exactly, maxima unchanged)
  for (int e = t; e < (KF - K) * LP; e += SC_NT) lg[K * LP + e] = -1e30f;
  __syncthreads();
  // pass 1: the two row-interpolated columns per class (registers, log2 units), the bound
  const float* la = lg + cc;
  const float* lb = lg + SC_LW + cc;
  const float wa2 = wtop * LOG2E, wb2 = wbot * LOG2E;
  float ml[KF], mr[KF];
  float M = -INFINITY;
#pragma unroll
  for (int k = 0; k < KF; ++k) {
    ml[k] = __builtin_fmaf(wa2, la[k * LP], wb2 * lb[k * LP]);
    mr[k] = __builtin_fmaf(wa2, la[k * LP + 1], wb2 * lb[k * LP + 1]);
    M = fmaxf(M, fmaxf(ml[k], mr[k]));
  }
  // pass 2: the softmax denominators under the shared upper-bound shift
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
  // a pixel whose own maximum lies far below the bound underflowed: redo it with its own maximum
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
  float inv[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) inv[j] = lv[j] >= 0 ? 1.f / sv[j] : 0.f;
  // per pixel: pl = its loss, pn = its share of the normaliser, pc = the factor on (p - onehot)
  float pl[4], pn[4], pc[4], Sj[4];
  {
    float nll[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      nll[j] = lv[j] >= 0 ? target_nll(la, lb, (lv[j] >= 0 ? lv[j] : 0) * LP, wa2, wb2, cl[j], cr[j], shv[j], sv[j])
                          : 0.f;
    if constexpr (LK == LK_CE) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        pc[j] = 1.f;
        pl[j] = nll[j];
        pn[j] = 1.f;
      }
    } else if constexpr (LK == LK_WCE) {
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
      // pass 2b: sum_k u_k p_k and the focal loss, over the K real classes (loss_cells.h)
      float fl[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) Sj[j] = fl[j] = 0.f;
#pragma unroll
      for (int k = 0; k < KF; ++k) {
        const bool real = k < K;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float e = __builtin_amdgcn_exp2f(__builtin_fmaf(cl[j], ml[k], __builtin_fmaf(cr[j], mr[k], -shv[j])));
          float p, u, lt;
          focal_class<GP>(e, sv[j], inv[j], k == lv[j], gamma, alpha, p, u, lt);
          Sj[j] += real ? u * p : 0.f;
          fl[j] += real ? lt : 0.f;
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) asm volatile("" : "+v"(Sj[j]), "+v"(fl[j]));   // complete here (loss_cells.h)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        pc[j] = cs;
        pl[j] = __builtin_fmaf(fs, fl[j], cs * nll[j]);
        pn[j] = 1.f;
      }
    }
  }
  // the loss of the cell's valid pixels (every pixel of the image lies in exactly one cell)
  {
    float ls = 0.f, lc = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      ls += lv[j] >= 0 ? pl[j] : 0.f;
      lc += lv[j] >= 0 ? pn[j] : 0.f;
    }
    ls = wave_sum(ls);
    lc = wave_sum(lc);
    if ((t & 63) == 0) {
      red[0][t >> 6] = ls;
      red[1][t >> 6] = lc;
    }
  }
  // pass 3: the gradient's x-adjoint: the 4 pixels' two column sums per class, the -onehot term taken at
  // the pixel's class inside the loop; the S / 4 threads of the cell row add theirs by the butterfly and the
  // first of them writes the row
  float* trow = t1 + rowi * 2 * SC_KP;
  float tj[4];                                    // the factor on -onehot; an invalid pixel: lv = -1 matches no class
#pragma unroll
  for (int j = 0; j < 4; ++j) tj[j] = pc[j];
  if constexpr (LK == LK_FOCAL) {
#pragma unroll
    for (int j = 0; j < 4; ++j) asm volatile("" : "+v"(shv[j]), "+v"(lv[j]));     // loss_cells.h: no carry-over
#pragma unroll
    for (int k = 0; k < KF; ++k) {
      float gl = 0.f, gr = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float e = __builtin_amdgcn_exp2f(__builtin_fmaf(cl[j], ml[k], __builtin_fmaf(cr[j], mr[k], -shv[j])));
        float p, u, lt;
        focal_class<GP>(e, sv[j], inv[j], k == lv[j], gamma, alpha, p, u, lt);
        const float g = __builtin_fmaf(p, __builtin_fmaf(fs, u - Sj[j], cs), k == lv[j] ? -tj[j] : 0.f);
        gl = __builtin_fmaf(cl[j], g, gl);
        gr = __builtin_fmaf(cr[j], g, gr);
      }
      gl = group_sum(gl, SEG);
      gr = group_sum(gr, SEG);
      if (seg == 0) {
        trow[k] = gl;
        trow[SC_KP + k] = gr;
      }
    }
  } else {
    float ai[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) ai[j] = inv[j] * pc[j];
#pragma unroll
    for (int k = 0; k < KF; ++k) {
      float gl = 0.f, gr = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float e = __builtin_amdgcn_exp2f(__builtin_fmaf(cl[j], ml[k], __builtin_fmaf(cr[j], mr[k], -shv[j])));
        const float g = __builtin_fmaf(ai[j], e, k == lv[j] ? -tj[j] : 0.f);
        gl = __builtin_fmaf(cl[j], g, gl);
        gr = __builtin_fmaf(cr[j], g, gr);
      }
      gl = group_sum(gl, SEG);
      gr = group_sum(gr, SEG);
      if (seg == 0) {
        trow[k] = gl;
        trow[SC_KP + k] = gr;
      }
    }
  }
  __syncthreads();
  if (t == 0) {
    float a = 0.f, n = 0.f;
#pragma unroll
    for (int i = 0; i < SC_NT / 64; ++i) {
      a += red[0][i];
      n += red[1][i];
    }
    part[(long)blockIdx.x * 2] = a;
    part[(long)blockIdx.x * 2 + 1] = n;
  }
  // y-adjoint: per cell, corner q = 2 * bottom + right and class, the S rows in row order
  for (int e = t; e < CPW * 4 * KF; e += SC_NT) {
    const int k = e % KF, q = (e / KF) & 3, ce = e / (4 * KF);
    if (k >= K || c0 + ce > w) continue;
    const float* tc = t1 + (ce * S) * 2 * SC_KP + (q & 1) * SC_KP + k;
    const float* wr = &wrow[ce * S][q >> 1];
    float acc = 0.f;
    for (int i = 0; i < S; ++i) acc = __builtin_fmaf(wr[2 * i], tc[i * 2 * SC_KP], acc);
    cell[((((long)b * (h + 1) + r) * (w + 1) + c0 + ce) * 4 + q) * KF + k] = acc;
  }
}

// adj (B, h, w, K): low-res pixel (y, x) is the bottom-right corner of cell (y, x), the bottom-left of
// (y, x + 1), the top-right of (y + 1, x) and the top-left of (y + 1, x + 1)
__global__ __launch_bounds__(256) void loss_scaled_gather(const float* __restrict__ cell, float* __restrict__ adj,
                                                          long n, int h, int w, int K) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int k = (int)(i % K), x = (int)((i / K) % w), y = (int)((i / ((long)K * w)) % h);
  const long b = i / ((long)K * w * h);
  const float* cb = cell + ((b * (h + 1) + y) * (w + 1) + x) * 4 * KF + k;
  const long rs = (long)(w + 1) * 4 * KF;
  const float a3 = cb[3 * KF], a2 = cb[4 * KF + 2 * KF], a1 = cb[rs + KF], a0 = cb[rs + 4 * KF];
  adj[i] = (a3 + a2) + (a1 + a0);
}

template <typename T, int LK, int GP>
void loss_scaled_launch(const T* logits, const int64_t* label, const float* cw, float* cell, float* part, int B, int h,
                        int w, int S, int K, int ignore, float gamma, float alpha, float cs, float fs, hipStream_t s) {
  const int gx = scaled_groups_x(w, S);
  hipLaunchKernelGGL((loss_scaled_cells<T, LK, GP>), dim3((unsigned)scaled_nblk(B, h, w, S)), dim3(SC_NT), 0, s, logits,
                     label, cw, cell, part, h, w, S, K, ignore, gamma, alpha, cs, fs, gx);
}

}  // namespace

extern "C" {

size_t cmx_upsample_loss_scaled_workspace(int B, int h, int w, int S) {
  if (B <= 0 || h <= 0 || w <= 0 || !scaled_ok(S)) return 0;
  return ((size_t)scaled_nblk(B, h, w, S) * 2 + (size_t)B * (h + 1) * (w + 1) * 4 * KF) * sizeof(float);
}

int cmx_upsample_loss_scaled_fwd_adj(const void* logits, const int64_t* label, const float* class_weight, float* adj,
                                     float* out, float* workspace, int B, int h, int w, int S, int K, int ignore_index,
                                     int kind, float gamma, float alpha, float ce_scale, float focal_scale, int dtype,
                                     hipStream_t s) {
  CMX_REQUIRE(B > 0 && h > 0 && w > 0 && scaled_ok(S) && K > 0 && K <= KF, CMX_ERR_SHAPE,
              "upsample_loss_scaled_fwd_adj: needs S in {8, 16, 32}, K <= %d (S=%d, K=%d, B=%d, %dx%d)", KF, S, K, B, h,
              w);
  CMX_REQUIRE((long)B * (h + 1) * scaled_groups_x(w, S) < (1L << 31) && (long)B * h * S * w * S < (1L << 40),
              CMX_ERR_SHAPE, "upsample_loss_scaled_fwd_adj: B=%d, %dx%d at S=%d is too large", B, h, w, S);
  CMX_REQUIRE(kind >= LK_CE && kind <= LK_FOCAL, CMX_ERR_ARG,
              "upsample_loss_scaled_fwd_adj: kind %d (-1 CE, 0 weighted CE, 1 FocalLoss2d, 2 ce_scale CE + focal_scale "
              "FocalLoss)", kind);
  CMX_REQUIRE(kind != LK_FOCAL || ((gamma == 0.f || gamma >= 1.f) && !class_weight), CMX_ERR_ARG,
              "upsample_loss_scaled_fwd_adj: FocalLoss takes gamma == 0 or gamma >= 1 (%g) and no class weight",
              (double)gamma);
  CMX_REQUIRE(kind != LK_CE || !class_weight, CMX_ERR_ARG,
              "upsample_loss_scaled_fwd_adj: kind -1 takes no class weight (kind 0 is the weighted CE)");
  CMX_REQUIRE(logits && label && adj && out && workspace, CMX_ERR_ARG, "upsample_loss_scaled_fwd_adj: null operand");
  CMX_REQUIRE(dtype >= 0 && dtype <= 2, CMX_ERR_DTYPE, "unsupported dtype %d", dtype);
  const uintptr_t la = dtype == 0 ? 3 : 1;
  CMX_REQUIRE(((uintptr_t)logits & la) == 0 && ((uintptr_t)label & 7) == 0 && ((uintptr_t)adj & 3) == 0 &&
                  ((uintptr_t)out & 3) == 0 && ((uintptr_t)workspace & 3) == 0 && ((uintptr_t)class_weight & 3) == 0,
              CMX_ERR_ARG, "upsample_loss_scaled_fwd_adj: a base is not aligned to its element");
  const long nb = scaled_nblk(B, h, w, S);
  float* part = workspace;
  float* cell = workspace + nb * 2;
#define CMX_SLOSS_LAUNCH(LK, GP)                                                                                      \
  CMX_DISPATCH(dtype, T, {                                                                                            \
    loss_scaled_launch<T, LK, GP>((const T*)logits, label, class_weight, cell, part, B, h, w, S, K, ignore_index,     \
                                  gamma, alpha, ce_scale, focal_scale, s);                                            \
  })
  if (kind == LK_CE) CMX_SLOSS_LAUNCH(LK_CE, 0);
  else if (kind == LK_WCE) CMX_SLOSS_LAUNCH(LK_WCE, 0);
  else if (kind == LK_FL2D) CMX_SLOSS_LAUNCH(LK_FL2D, 0);
  else if (gamma == 0.f) CMX_SLOSS_LAUNCH(LK_FOCAL, 0);
  else if (gamma == 1.f) CMX_SLOSS_LAUNCH(LK_FOCAL, 1);
  else if (gamma == 2.f) CMX_SLOSS_LAUNCH(LK_FOCAL, 2);
  else if (gamma == 4.f) CMX_SLOSS_LAUNCH(LK_FOCAL, 4);
  else CMX_SLOSS_LAUNCH(LK_FOCAL, GP_GEN);
#undef CMX_SLOSS_LAUNCH
  const long n = (long)B * h * w * K;
  hipLaunchKernelGGL(loss_scaled_gather, dim3(cdiv(n, 256)), dim3(256), 0, s, cell, adj, n, h, w, K);
  if (kind == LK_FOCAL && ce_scale == 0.f)
    hipLaunchKernelGGL(loss_finalize_kernel<true>, dim3(1), dim3(256), 0, s, part, (int)nb, out);
  else
    hipLaunchKernelGGL(loss_finalize_kernel<false>, dim3(1), dim3(256), 0, s, part, (int)nb, out);
  return cmx_check_launch("upsample_loss_scaled_fwd_adj");
}

}  // extern "C"
