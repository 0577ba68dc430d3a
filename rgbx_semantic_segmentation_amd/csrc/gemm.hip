// Batched MFMA GEMM with fused epilogues for every dense layer of the step.
//
//   C[g](i, j) = epi( sum_k A[g](i, k) * B[g](j, k) )          g < G, i < M, j < N, k < K
//
// A(i, k) is read from A[i*lda + k] (transA = 0, k contiguous) or A[k*lda + i] (transA = 1,
// i contiguous); likewise B.  The three GEMMs of a Linear / 1x1 conv / im2col conv are
//   forward   y  = x W^T   : A = x (M x K),  B = W (N x K)           transA = 0, transB = 0
//   dgrad     dx = dy W    : A = dy (M x N), B(j=k', k=n) = W[n][k']  transA = 0, transB = 1
//   wgrad     dW = dy^T x  : A(i=n, k=m) = dy[m][n], B(j=k', k=m) = x[m][k']   both 1
// (reference layers: dual_segformer.py Linear/Conv2d, net_utils.py 1x1 convs, MLPDecoder.py).
//
// Extras that remove whole passes / launches from the step:
//  * two-segment A along k (k < K1 from A, k >= K1 from A2): Linear on cat(x1, x2) without
//    the cat (CrossPath.end_proj, ChannelEmbed, net_utils.py:277-280, 323-326);
//  * `ones_col`: column N - 1 of the result is sum_k A(i, k) (the bias gradient of a wgrad,
//    sum over tokens of dy), routed to `dbias` -- no colsum launch;
//  * split-K over blockIdx.z into fp32 partial slabs + a reducer that applies the full
//    epilogue: the wgrads reduce over up to 76800 tokens into a 64 x 256 result, and the
//    stage-4 layers (600 tokens) have only ~20 output tiles; both need K parallelism.
//
// Epilogue (per output element, fp32):  v = acc + bias[j];  v = act(v);
//   out_mode 0: C = T(v)            out_mode 1: C = fp32(v)        out_mode 2: C += v (fp32)
//   residual R (same layout as C):  C = R + s[(g*M + i) / rows_per_sample] * v  (DropPath-scaled
//   residual, s may be NULL = 1) -- the Block's `x + drop_path(f(x))` (dual_segformer.py:168-169).
//
// Two kernels:
//  * gemm_bf16_kernel -- the bf16 path of the step.  256 threads = 4 waves (2 x 2) over a
//    BM x BN tile (64 or 128 each), v_mfma_f32_32x32x16_bf16, BK = 64.  Operand tiles move
//    HBM -> LDS by buffer_load_dwordx4 ... lds (LDS-DMA, no register staging), double
//    buffered: tile t+1 is in flight while tile t is multiplied.  Out-of-range rows / k come
//    back as zeros from the buffer descriptor's range check (offset 0x80000000), so ragged
//    edges need no branches.  A k-contiguous operand is imaged [rows][64] (128-B rows) and
//    read with ds_read_b128; a row-contiguous (transposed) operand is imaged [64][rows] and
//    read with gfx950's ds_read_b64_tr_b16, which transposes 4 x 16 blocks on the way to the
//    registers -- no transposing LDS writes.  Both images are XOR-swizzled on 16-B chunks so
//    every fragment read is bank-conflict-free; the LDS-DMA writes linearly, so the inverse
//    swizzle is applied to the per-lane global source address.
//  * gemm_generic_kernel -- fp32 parity mode (exact v_mfma_f32_32x32x2_f32) and any bf16
//    problem whose strides / dims do not allow 16-B chunks; register staged, BK = 32.
#include "gemm_kernels.h"
#include <string.h>
#include <stdlib.h>

using namespace gemmk;
namespace gp = gemmplan;
extern CMX_GEMM_FAST_INST(bf16)
extern CMX_GEMM_FAST_INST(f16)
extern CMX_GEMM_GENERIC_INST(float)
extern CMX_GEMM_GENERIC_INST(bf16)
extern CMX_GEMM_GENERIC_INST(f16)
static_assert(gp::FAST_BK == FBK && gp::GENERIC_BK == BK, "gemm_plan.h counts k-tiles of the kernels' depth");

namespace {
// the launch-policy knobs as they stand now: read at every planned launch (eager call or graph
// capture), so a cmx_tune takes effect at the next one
gp::GemmKnobs gemm_knobs() {
  gp::GemmKnobs k;                               // (the defaults)
  k.tiles = cmx_knob("GEMM_TILES", k.tiles);
  k.smallk = cmx_knob("GEMM_SMALLK", k.smallk);
  k.t128 = cmx_knob("GEMM_T128", k.t128);
  k.splitkw = cmx_knob("GEMM_SPLITKW", k.splitkw);
  k.kw = cmx_knob("GEMM_KW", k.kw);
  k.mid = cmx_knob("GEMM_MID", k.mid);
  k.stream = cmx_knob("GEMM_STREAM", k.stream);
  k.stream_k = cmx_knob("GEMM_STREAM_K", k.stream_k);
  k.stream_bpc = cmx_knob("GEMM_STREAM_BPC", k.stream_bpc);
  k.grouped_kt = cmx_knob("GROUPED_KT", k.grouped_kt);
  return k;
}

// the kernel(s) a plan names: the one place a GemmLaunch becomes launches
int launch_gemm(const gp::GemmLaunch& L, const GemmArgs& a, int tA, int tB, int dtype, hipStream_t s) {
  bool ok = true;
  if (L.path == gp::PATH_STREAM) {
    if (dtype == 2) launch_stream<f16>(L, a, tB, s);
    else launch_stream<bf16>(L, a, tB, s);
  } else if (L.path == gp::PATH_TILE) ok = dtype == 2 ? launch_tile<f16>(L, a, tA, tB, s) : launch_tile<bf16>(L, a, tA, tB, s);
  else if (dtype == 1) ok = launch_generic<bf16>(L, a, tA, tB, s);
  else if (dtype == 2) ok = launch_generic<f16>(L, a, tA, tB, s);
  else ok = launch_generic<float>(L, a, tA, tB, s);
  CMX_REQUIRE(ok, CMX_ERR_LAUNCH, "gemm: no kernel for path %d, tile %d x %d, NS %d, KW %d", L.path, L.bm, L.bn, L.ns,
              L.kw);
  if (L.nsplit > 1) {
    if (dtype == 1) launch_reduce<bf16>(L, a, s);
    else if (dtype == 2) launch_reduce<f16>(L, a, s);
    else launch_reduce<float>(L, a, s);
  }
  return CMX_OK;
}

// the plan's share of the kernel arguments
void set_plan(GemmArgs& a, const gp::GemmLaunch& L) {
  a.kt_per_split = L.kt_per_split; a.nsplit = L.nsplit; a.tiles_m = L.tiles_m; a.tiles_n = L.tiles_n;
}

// ============================================================================ grouped reduce
// out (+)= sum over nblk partial rows, for many reductions in one launch: the split-K slabs of
// the grouped weight gradients, the per-block dgamma / dbeta partials of LayerNorm backward and
// the dW / db partials of the depthwise conv backward.  Element w < rows * cols of group g is
// sum_b src[g*sg + b*sb + w]; it lands at dst[g*dg + r*ldd + c] (c < csplit) or
// dst2[g*dg2 + r*ldd2 + c - csplit] (r = w / cols, c = w % cols): e.g. LN's [dgamma | dbeta]
// rows, DWConv's [9 taps | bias] rows, a GEMM slab's row pitch vs the gradient view's ldc.
// zl threads share one output along b (long partial columns), meeting in LDS.
struct RedRec {
  const float* src; float* dst; float* dst2;
  long sg, sb, dg, dg2;
  int ldd, ldd2, G, nblk, rows, cols, csplit, accumulate, zl, cpg, blk0, pad;
};

__global__ __launch_bounds__(256) void reduce_grouped_kernel(const RedRec* __restrict__ recs, int nrec) {
  __shared__ float red[256];
  const int b = blockIdx.x;
  int lo = 0, hi = nrec - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (recs[mid].blk0 <= b) lo = mid; else hi = mid - 1;
  }
  const RedRec& r = recs[lo];
  const int zl = r.zl, opb = 256 / zl;
  const int local = b - r.blk0;
  const int g = local / r.cpg, ch = local % r.cpg;
  const int o = threadIdx.x % opb, sl = threadIdx.x / opb;
  const long W = (long)r.rows * r.cols;
  const long w = (long)ch * opb + o;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (w < W) {
    const float* p = r.src + (long)g * r.sg + w;
    const long sb = r.sb;
    int k = sl;
    for (; k + 3 * zl < r.nblk; k += 4 * zl) {
      s0 += p[(long)k * sb];
      s1 += p[(long)(k + zl) * sb];
      s2 += p[(long)(k + 2 * zl) * sb];
      s3 += p[(long)(k + 3 * zl) * sb];
    }
    for (; k < r.nblk; k += zl) s0 += p[(long)k * sb];
  }
  float v = (s0 + s1) + (s2 + s3);
  if (zl > 1) {
    red[threadIdx.x] = v;
    __syncthreads();
    if (sl) return;
    for (int q = 1; q < zl; ++q) v += red[o + q * opb];
  }
  if (w >= W) return;
  const int row = (int)(w / r.cols), c = (int)(w % r.cols);
  float* d = c < r.csplit ? r.dst + (long)g * r.dg + (long)row * r.ldd + c
                          : r.dst2 + (long)g * r.dg2 + (long)row * r.ldd2 + (c - r.csplit);
  *d = r.accumulate ? *d + v : v;
}

}  // namespace

extern "C" {

size_t cmx_gemm_workspace(int G, int M, int N, int splitk) {
  return splitk > 1 ? (size_t)G * splitk * M * N * sizeof(float) : 0;
}

int cmx_gemm_splitk(int G, int M, int N, int K, int ones_col, int dtype) {
  return gp::default_split(G, M, N, K, ones_col, dtype, gemm_knobs());
}

}  // extern "C"

namespace {
// a planned problem for cmx_gemm_multi (host memory of cmx_gemm_plan_size() bytes)
struct GemmPlan {
  GemmArgs a;
  int tA, tB, dtype, nblk, nk64, pad;
};

// LayerNorm of the output rows in the epilogue (cmx_gemm_ln)
struct LnTail {
  const float* gamma; const float* beta; long sg; void* y; float* mean; float* rstd; float eps;
};

// LayerNorm backward of the epilogue (cmx_gemm_ln_bwd)
struct LnBwd {
  const void* x; const float* gamma; long sg; const float* mean; const float* rstd; const void* dy2; void* dxs;
  float* part;
};

// upsample-add sources of the epilogue (nup = 0: none)
struct UpSpec {
  const void* src[3];
  int h[3], w[3], n, oH, oW;
};

// one GEMM as an entry point describes it; an entry point names the fields it uses, the rest
// keep these defaults
struct GemmProblem {
  const void* A = nullptr; const void* A2 = nullptr; const void* B = nullptr; void* C = nullptr;
  const float* bias = nullptr; const void* R = nullptr; const float* rscale = nullptr; const void* mask = nullptr;
  float* dbias = nullptr; float* workspace = nullptr;
  int G = 0, M = 0, N = 0, K = 0, K1 = 0;                          // (K1: used with A2 only)
  int64_t lda = 0, lda2 = 0, ldb = 0, ldc = 0, sA = 0, sA2 = 0, sB = 0, sC = 0, sbias = 0, sdb = 0;
  int rows_per_sample = 1, transA = 0, transB = 0, act = 0, out_mode = 0, ones_col = 0;
  int splitk = 0, dtype = 0;
  int scR = 0, scH = 0, scW = 0, scC = 0, scHo = 0, scWo = 0;      // patch-scatter epilogue (scR > 0)
  int gh = 1;                                                      // two-level batch
  int64_t sAh = 0, sBh = 0, sCh = 0;
  const UpSpec* up = nullptr;
  const LnTail* tail = nullptr;
  const LnBwd* lnb = nullptr;
  GemmPlan* plan = nullptr;                                        // plan only, nothing launched (cmx_gemm_plan)
};

int gemm_impl(const GemmProblem& p, hipStream_t s) {
  const int G = p.G, M = p.M, N = p.N, K = p.K, dtype = p.dtype, out_mode = p.out_mode, ones_col = p.ones_col;
  const int transA = p.transA, transB = p.transB, gh = p.gh;
  const LnTail* tail = p.tail;
  const LnBwd* lnb = p.lnb;
  const UpSpec* up = p.up;
  CMX_REQUIRE(G > 0 && M > 0 && N > 0 && K > 0, CMX_ERR_SHAPE, "gemm: empty problem G=%d M=%d N=%d K=%d", G, M, N, K);
  CMX_REQUIRE(dtype >= 0 && dtype <= 2, CMX_ERR_DTYPE, "gemm: unsupported dtype %d", dtype);
  CMX_REQUIRE(out_mode >= 0 && out_mode <= 2 && p.act >= 0 && p.act <= 3, CMX_ERR_ARG, "gemm: out_mode/act");
  CMX_REQUIRE(!(p.R && out_mode == 2), CMX_ERR_ARG, "gemm: residual with accumulate");
  const int K1 = p.A2 ? p.K1 : K;
  CMX_REQUIRE(K1 > 0 && K1 <= K && (K1 == K || !transA), CMX_ERR_SHAPE,
              "gemm: a second A segment needs transA = 0 (K1=%d K=%d)", K1, K);
  CMX_REQUIRE(!p.R || p.rows_per_sample > 0, CMX_ERR_ARG, "gemm: rows_per_sample");
  CMX_REQUIRE(!ones_col || (transB && p.dbias && N >= 2 && out_mode != 0 && !p.bias && !p.R && p.act == 0), CMX_ERR_ARG,
              "gemm: ones_col (bias gradient) needs transB, dbias, fp32 output and no epilogue");
  CMX_REQUIRE((long)M * N < (1L << 31) && (long)M * K < (1L << 40), CMX_ERR_SHAPE, "gemm: problem too large");
  const bool fast = dtype != 0 && fast_ok(p.A, p.A2, p.B, M, N, K, K1, p.lda, p.lda2, p.ldb, p.sA, p.sA2, p.sB, transA,
                                          transB, ones_col) && p.sAh % 8 == 0 && p.sBh % 8 == 0;
  const int V = dtype == 0 ? 4 : 8;
  const int nb = ones_col ? N - 1 : N;
  const bool vec = (transA ? M : K) % V == 0 && (transB ? nb : K) % V == 0 && (K - K1) % V == 0 && (K1 == K || K1 % V == 0) &&
                   p.lda % V == 0 && p.ldb % V == 0 && p.sA % V == 0 && p.sB % V == 0 &&
                   (!p.A2 || (p.lda2 % V == 0 && p.sA2 % V == 0)) && ((uintptr_t)p.A % 16 == 0) &&
                   ((uintptr_t)p.B % 16 == 0) && (!p.A2 || (uintptr_t)p.A2 % 16 == 0);
  CMX_REQUIRE(fast || K1 == K || K1 % BK == 0, CMX_ERR_SHAPE, "gemm: second A segment needs K1 %% %d == 0", BK);
  const int nup = up && up->n > 0 ? up->n : 0;
  gp::GemmShape shape;
  shape.G = G; shape.M = M; shape.N = N; shape.K = K; shape.transA = transA; shape.transB = transB;
  shape.ones_col = ones_col; shape.dtype = dtype; shape.fast = fast; shape.splitk = p.splitk; shape.a2 = p.A2 != nullptr;
  shape.row_ln = tail != nullptr; shape.ln_bwd = lnb != nullptr; shape.scC = p.scR > 0 ? p.scC : 0; shape.nup = nup;
  shape.gh = gh; shape.tile_only = p.plan != nullptr;
  const gp::GemmLaunch L = plan_gemm(shape, gemm_knobs(), cu_count());
  const int splitk = L.nsplit;
  CMX_REQUIRE((p.splitk > 0 ? p.splitk : splitk) == 1 || p.workspace, CMX_ERR_ARG, "gemm: split-K needs a workspace");
  GemmArgs a{};
  a.A = p.A; a.A2 = p.A2; a.B = p.B; a.C = p.C; a.bias = p.bias; a.R = p.R; a.rscale = p.rscale; a.dbias = p.dbias;
  a.ws = p.workspace;
  a.G = G; a.M = M; a.N = N; a.K = K; a.K1 = K1; a.rows_per_sample = p.rows_per_sample > 0 ? p.rows_per_sample : 1;
  a.act = p.act; a.out_mode = out_mode; a.ones_col = ones_col; a.vec = vec;
  CMX_REQUIRE(!p.mask || (out_mode == 0 && !ones_col && (uintptr_t)p.mask % 16 == 0 && (!p.R || p.R != p.mask)),
              CMX_ERR_ARG, "gemm: a ReLU mask needs a plain store in C's layout");
  a.mask = p.mask;
  // 8-column epilogue groups as aligned vectors: C (and R) rows start on 16-B boundaries
  const long esz = out_mode == 0 ? (dtype != 0 ? 2 : 4) : 4;
  a.cvec = ((uintptr_t)p.C % 16 == 0) && (p.ldc * esz) % 16 == 0 && (p.sC * esz) % 16 == 0 &&
           (!p.R || (uintptr_t)p.R % 16 == 0);
  a.lda = p.lda; a.lda2 = p.lda2; a.ldb = p.ldb; a.ldc = p.ldc; a.sA = p.sA; a.sA2 = p.sA2; a.sB = p.sB; a.sC = p.sC;
  a.sbias = p.sbias; a.sdb = p.sdb;
  CMX_REQUIRE(gh >= 1 && (gh == 1 || (G % gh == 0 && !p.A2 && !p.bias && !p.R && !ones_col && !nup && !p.scR)),
              CMX_ERR_ARG, "gemm: a two-level batch (gh=%d) takes G %% gh == 0 and no A2 / bias / residual / "
              "bias-gradient / upsample / scatter", gh);
  a.gh = gh; a.sAh = p.sAh; a.sBh = p.sBh; a.sCh = p.sCh;
  if (nup) {
    CMX_REQUIRE(up->n <= 3 && G == 1 && !ones_col && N % 8 == 0 && (long)up->oH * up->oW > 0 &&
                M % (up->oH * up->oW) == 0, CMX_ERR_ARG, "gemm: upsample-add epilogue needs G = 1, N %% 8 == 0 and "
                "M a whole number of %d x %d grids", up->oH, up->oW);
    for (int q = 0; q < up->n; ++q) {
      CMX_REQUIRE(up->src[q] && ((uintptr_t)up->src[q] & 15) == 0 && up->h[q] > 0 && up->w[q] > 0, CMX_ERR_ARG,
                  "gemm: upsample-add source %d", q);
      a.up[q] = up->src[q]; a.uh[q] = up->h[q]; a.uw[q] = up->w[q];
    }
    a.nup = up->n; a.uoH = up->oH; a.uoW = up->oW;
  }
  if (p.scR > 0) {
    CMX_REQUIRE(G == 1 || p.sC > 0, CMX_ERR_ARG, "gemm: scatter");
    CMX_REQUIRE((!p.R || lnb) && out_mode == 0 && !ones_col && N == p.scR * p.scR * p.scC && M % (p.scHo * p.scWo) == 0,
                CMX_ERR_ARG, "gemm: patch scatter needs a plain store of N = R*R*C columns");
    a.scatter = 1; a.scH = p.scH; a.scW = p.scW; a.scC = p.scC; a.scR = p.scR; a.scHo = p.scHo; a.scWo = p.scWo;
  }
  set_plan(a, L);
  // LayerNorm of C's rows in the same launch (tail = 2): N <= 128, one 64 x 64 / 64 x 128 tile
  // spans the row and the lanes that store it normalise it
  if (tail) {
    CMX_REQUIRE(fast && N <= 128 && N % 8 == 0 && splitk == 1 && !transA && !transB && out_mode == 0 && !ones_col &&
                    !a.nup && !a.scatter && gh == 1 && !p.mask && a.cvec && dtype != 0,
                CMX_ERR_ARG, "gemm_ln: the LayerNorm epilogue needs the 16-bit path without split-K, forward layouts, a "
                "plain aligned store and N <= 128, N %% 8 == 0 (G=%d M=%d N=%d K=%d)", G, M, N, K);
    CMX_REQUIRE(tail->gamma && tail->beta && tail->y && tail->mean && tail->rstd && ((uintptr_t)tail->y & 15) == 0 &&
                    tail->y != p.C, CMX_ERR_ARG, "gemm_ln: LayerNorm buffers");
    a.tail = 2; a.ln_gamma = tail->gamma; a.ln_beta = tail->beta; a.ln_sg = tail->sg; a.ln_y = tail->y;
    a.ln_mean = tail->mean; a.ln_rstd = tail->rstd; a.ln_eps = tail->eps;
  }
  if (lnb) {
    const bool al = ((uintptr_t)p.C & 15) == 0 && ((uintptr_t)lnb->x & 15) == 0 && ((uintptr_t)p.R & 15) == 0 &&
                    ((uintptr_t)lnb->dy2 & 15) == 0 && ((uintptr_t)lnb->dxs & 15) == 0;
    // (under the patch scatter a 64 x C tile is one tap of 64 patches: C must be a tile width)
    const bool rows_ok = a.scatter ? (p.scC == 64 || p.scC == 128) && p.scH == p.scHo * p.scR && p.scW == p.scWo * p.scR
                                   : N <= 128 && N % 8 == 0;
    CMX_REQUIRE(fast && splitk == 1 && !transA && transB && out_mode == 0 && !ones_col && !p.bias && p.act == 0 &&
                    !p.mask && !a.nup && gh == 1 && !p.A2 && a.cvec && al && rows_ok && dtype != 0 &&
                    !tail && lnb->x && lnb->gamma && lnb->mean && lnb->rstd && lnb->part && (!lnb->dxs || p.rscale),
                CMX_ERR_ARG, "gemm_ln_bwd: needs the 16-bit dgrad path (transB) without split-K, 16-B aligned rows, "
                "N <= 128 (N %% 8 == 0), no bias / activation (G=%d M=%d N=%d K=%d)", G, M, N, K);
    a.tail = 3; a.ln_gamma = lnb->gamma; a.ln_sg = lnb->sg; a.ln_mean = const_cast<float*>(lnb->mean); a.ln_rstd = const_cast<float*>(lnb->rstd);
    a.lnb_x = lnb->x; a.lnb_dy2 = lnb->dy2; a.lnb_dxs = lnb->dxs; a.lnb_part = lnb->part;
  }
  if (p.plan) {
    // planning only (cmx_gemm_plan): the block count when eligible for a multi launch, else 0
    const int nblk = gp::multi_blocks(shape, L);
    if (!nblk) return 0;
    a.kt_per_split = (int)gp::cdiv(K, FBK);      // (cmx_gemm_multi sets the k-group's share)
    memset(p.plan, 0, sizeof(*p.plan));
    p.plan->a = a; p.plan->tA = transA; p.plan->tB = transB; p.plan->dtype = dtype;
    p.plan->nblk = nblk;
    p.plan->nk64 = a.kt_per_split;
    return nblk;
  }
  const int st = launch_gemm(L, a, transA, transB, dtype, s);
  return st != CMX_OK ? st : cmx_check_launch("gemm");
}
}  // namespace

extern "C" {

int cmx_gemm(const void* A, const void* A2, const void* B, void* C, const float* bias, const void* R,
             const float* rscale, const void* mask, float* dbias, float* workspace, int G, int M, int N, int K, int K1,
             int64_t lda, int64_t lda2, int64_t ldb, int64_t ldc, int64_t sA, int64_t sA2, int64_t sB, int64_t sC,
             int64_t sbias, int64_t sdb, int rows_per_sample, int transA, int transB, int act, int out_mode,
             int ones_col, int splitk, int dtype, hipStream_t s) {
  GemmProblem p;
  p.A = A; p.A2 = A2; p.B = B; p.C = C; p.bias = bias; p.R = R; p.rscale = rscale; p.mask = mask; p.dbias = dbias;
  p.workspace = workspace; p.G = G; p.M = M; p.N = N; p.K = K; p.K1 = K1; p.lda = lda; p.lda2 = lda2; p.ldb = ldb;
  p.ldc = ldc; p.sA = sA; p.sA2 = sA2; p.sB = sB; p.sC = sC; p.sbias = sbias; p.sdb = sdb;
  p.rows_per_sample = rows_per_sample; p.transA = transA; p.transB = transB; p.act = act; p.out_mode = out_mode;
  p.ones_col = ones_col; p.splitk = splitk; p.dtype = dtype;
  return gemm_impl(p, s);
}

int cmx_gemm_ln(const void* A, const void* A2, const void* B, void* C, const float* bias, const void* R,
                const float* rscale, int G, int M, int N, int K, int K1, int64_t lda, int64_t lda2, int64_t ldb,
                int64_t ldc, int64_t sA, int64_t sA2, int64_t sB, int64_t sC, int64_t sbias, int rows_per_sample,
                int act, const float* ln_gamma, const float* ln_beta, int64_t ln_sg, float ln_eps, void* ln_y,
                float* ln_mean, float* ln_rstd, int dtype, hipStream_t s) {
  const LnTail t{ln_gamma, ln_beta, (long)ln_sg, ln_y, ln_mean, ln_rstd, ln_eps};
  GemmProblem p;
  p.A = A; p.A2 = A2; p.B = B; p.C = C; p.bias = bias; p.R = R; p.rscale = rscale;
  p.G = G; p.M = M; p.N = N; p.K = K; p.K1 = K1; p.lda = lda; p.lda2 = lda2; p.ldb = ldb; p.ldc = ldc;
  p.sA = sA; p.sA2 = sA2; p.sB = sB; p.sC = sC; p.sbias = sbias; p.rows_per_sample = rows_per_sample; p.act = act;
  p.splitk = 1; p.dtype = dtype; p.tail = &t;
  return gemm_impl(p, s);
}

int cmx_gemm_ln_bwd(const void* A, const void* B, void* dx, int G, int M, int N, int K, int64_t lda, int64_t ldb,
                    int64_t ldc, int64_t sA, int64_t sB, int64_t sC, const void* x, const float* gamma, int64_t sg,
                    const float* mean, const float* rstd, const void* dres, const void* dy2, const float* sscale,
                    int rows_per_sample, void* dxs, float* partials, int dtype, hipStream_t s) {
  const LnBwd l{x, gamma, (long)sg, mean, rstd, dy2, dxs, partials};
  GemmProblem p;
  p.A = A; p.B = B; p.C = dx; p.R = dres; p.rscale = sscale; p.G = G; p.M = M; p.N = N; p.K = K;
  p.lda = lda; p.ldb = ldb; p.ldc = ldc; p.sA = sA; p.sB = sB; p.sC = sC; p.rows_per_sample = rows_per_sample;
  p.transB = 1; p.splitk = 1; p.dtype = dtype; p.lnb = &l;
  return gemm_impl(p, s);
}


size_t cmx_gemm_ln_bwd_partials(int G, int M, int N) { return (size_t)G * ((M + 63) / 64) * 2 * N * sizeof(float); }

// cmx_conv_patch_dgrad with the backward of the LayerNorm that produced the conv's input in the
// epilogue: dx = LN'(col2im(dy W) [+ dy2]) + dres (the norm's input gradient), never storing the conv's
int cmx_conv_patch_dgrad_ln_bwd(const void* dy, const void* Wt, void* dx, int G, int NIg, int H, int Wd, int C, int R,
                                int Ho, int Wo, int N, int64_t sdy, int64_t sW, int64_t sdx, const void* x,
                                const float* gamma, int64_t sg, const float* mean, const float* rstd, const void* dres,
                                const void* dy2, const float* sscale, int rows_per_sample, void* dxs, float* partials,
                                int dtype, hipStream_t s) {
  CMX_REQUIRE(G > 0 && NIg > 0 && (C == 64 || C == 128) && R > 0 && Ho * R == H && Wo * R == Wd, CMX_ERR_SHAPE,
              "conv_patch_dgrad_ln_bwd: H=%d W=%d R=%d Ho=%d Wo=%d C=%d (exact patches, C 64 / 128)", H, Wd, R, Ho, Wo,
              C);
  const int M = NIg * Ho * Wo, Kc = R * R * C;
  const LnBwd l{x, gamma, (long)sg, mean, rstd, dy2, dxs, partials};
  GemmProblem p;
  p.A = dy; p.B = Wt; p.C = dx; p.R = dres; p.rscale = sscale; p.G = G; p.M = M; p.N = Kc; p.K = N;
  p.lda = N; p.ldb = Kc; p.ldc = Kc; p.sA = sdy; p.sB = sW; p.sC = sdx; p.rows_per_sample = rows_per_sample;
  p.transB = 1; p.splitk = 1; p.dtype = dtype; p.lnb = &l;
  p.scR = R; p.scH = H; p.scW = Wd; p.scC = C; p.scHo = Ho; p.scWo = Wo;
  return gemm_impl(p, s);
}

size_t cmx_conv_patch_dgrad_ln_bwd_partials(int G, int NIg, int Ho, int Wo, int C, int R) {
  return (size_t)G * ((NIg * Ho * Wo + 63) / 64) * R * R * 2 * C * sizeof(float);
}

size_t cmx_gemm_plan_size(void) { return sizeof(GemmPlan); }

// cmx_gemm's arguments, planned instead of launched: > 0 = the problem's block count (eligible
// for cmx_gemm_multi), 0 = not eligible (run it with cmx_gemm), < 0 = invalid arguments
int cmx_gemm_plan(void* plan, const void* A, const void* A2, const void* B, void* C, const float* bias, const void* R,
                  const float* rscale, const void* mask, float* dbias, float* workspace, int G, int M, int N, int K,
                  int K1, int64_t lda,
                  int64_t lda2, int64_t ldb, int64_t ldc, int64_t sA, int64_t sA2, int64_t sB, int64_t sC,
                  int64_t sbias, int64_t sdb, int rows_per_sample, int transA, int transB, int act, int out_mode,
                  int ones_col, int splitk, int dtype) {
  CMX_REQUIRE(plan, CMX_ERR_ARG, "gemm_plan: null plan");
  GemmProblem p;
  p.A = A; p.A2 = A2; p.B = B; p.C = C; p.bias = bias; p.R = R; p.rscale = rscale; p.mask = mask; p.dbias = dbias;
  p.workspace = workspace; p.G = G; p.M = M; p.N = N; p.K = K; p.K1 = K1; p.lda = lda; p.lda2 = lda2; p.ldb = ldb;
  p.ldc = ldc; p.sA = sA; p.sA2 = sA2; p.sB = sB; p.sC = sC; p.sbias = sbias; p.sdb = sdb;
  p.rows_per_sample = rows_per_sample; p.transA = transA; p.transB = transB; p.act = act; p.out_mode = out_mode;
  p.ones_col = ones_col; p.splitk = splitk; p.dtype = dtype; p.plan = reinterpret_cast<GemmPlan*>(plan);
  return gemm_impl(p, nullptr);
}

// n <= 4 planned problems (same dtype and B layout) in ONE launch; waves / ring depth chosen for
// the combined grid as a single problem's launch would be (gemm_plan.h: plan_multi)
int cmx_gemm_multi(const void* plans, int n, hipStream_t s) {
  CMX_REQUIRE(plans && n >= 1 && n <= MULTI_MAX, CMX_ERR_ARG, "gemm_multi: 1..%d problems (got %d)", MULTI_MAX, n);
  const GemmPlan* pl = reinterpret_cast<const GemmPlan*>(plans);
  GemmMulti m{};
  m.n = n;
  int total = 0, nk64 = 1 << 30;
  for (int i = 0; i < n; ++i) {
    CMX_REQUIRE(pl[i].nblk > 0 && pl[i].tA == 0 && pl[i].tB == pl[0].tB && pl[i].dtype == pl[0].dtype &&
                (pl[i].dtype == 1 || pl[i].dtype == 2), CMX_ERR_ARG, "gemm_multi: plan %d does not match plan 0", i);
    m.a[i] = pl[i].a;
    m.blk0[i] = total;
    total += pl[i].nblk;
    nk64 = nk64 < pl[i].nk64 ? nk64 : pl[i].nk64;
  }
  m.blk0[n] = total;
  for (int i = n + 1; i <= MULTI_MAX; ++i) m.blk0[i] = total;
  const gp::GemmLaunch L = gp::plan_multi(total, nk64, gemm_knobs());
  for (int i = 0; i < n; ++i) m.a[i].kt_per_split = gp::split_k(pl[i].nk64, L.kw).kt;
  const dim3 grid(L.grid_x), block(L.block);
  const bool tB = pl[0].tB != 0, h = pl[0].dtype == 2;
  bool ok = false;
#define CMX_GEMM_MULTI(NS, KW, TB, H, E)                                                       \
  if (L.ns == NS && L.kw == KW && tB == TB && h == H) {                                        \
    hipLaunchKernelGGL((gemm_multi_kernel<NS, KW, TB, E>), grid, block, 0, s, m);               \
    ok = true;                                                                                  \
  }
#define CMX_GEMM_MULTI_W(NS, KW) \
  CMX_GEMM_MULTI(NS, KW, false, false, bf16) CMX_GEMM_MULTI(NS, KW, true, false, bf16) \
  CMX_GEMM_MULTI(NS, KW, false, true, f16) CMX_GEMM_MULTI(NS, KW, true, true, f16)
  CMX_GEMM_MULTI_W(4, 2) CMX_GEMM_MULTI_W(2, 2) CMX_GEMM_MULTI_W(4, 1) CMX_GEMM_MULTI_W(2, 1)
#undef CMX_GEMM_MULTI_W
#undef CMX_GEMM_MULTI
  CMX_REQUIRE(ok, CMX_ERR_LAUNCH, "gemm_multi: no kernel for NS %d, KW %d", L.ns, L.kw);
  return cmx_check_launch("gemm_multi");
}

// dx of a non-overlapping patchify conv (stride == kernel == R, pad 0: Attention.sr,
// dual_segformer.py:95-96) in ONE launch: dx[g] = col2im(dy[g] @ W[g]) with the col2im folded
// into the GEMM epilogue as an address remap (every input pixel belongs to at most one patch,
// so there is no overlap to sum).  dy (G, NIg*Ho*Wo, N), W (G, N, R*R*C) tap-major, dx
// (G*NIg, H, W, C) NHWC.  Pixels outside the Ho*R x Wo*R window (H or W not a multiple of R)
// are not written: the caller zeroes dx for such shapes.
// cmx_gemm over a two-level batch: G = Go * gh problems, problem g = (g / gh, g % gh) at operand
// offsets (g / gh) * sX + (g % gh) * sXh (per-head products of the FFM cross attention:
// net_utils.py:206-212, (image x modality, head) pairs with the heads a column slice of a row)
int cmx_gemm_h2(const void* A, const void* B, void* C, float* workspace, int G, int gh, int M, int N, int K,
                int64_t lda, int64_t ldb, int64_t ldc, int64_t sA, int64_t sAh, int64_t sB, int64_t sBh, int64_t sC,
                int64_t sCh, int transA, int transB, int out_mode, int splitk, int dtype, hipStream_t s) {
  GemmProblem p;
  p.A = A; p.B = B; p.C = C; p.workspace = workspace; p.G = G; p.M = M; p.N = N; p.K = K;
  p.lda = lda; p.ldb = ldb; p.ldc = ldc; p.sA = sA; p.sB = sB; p.sC = sC; p.transA = transA; p.transB = transB;
  p.out_mode = out_mode; p.splitk = splitk; p.dtype = dtype; p.gh = gh; p.sAh = sAh; p.sBh = sBh; p.sCh = sCh;
  return gemm_impl(p, s);
}

int cmx_conv_patch_dgrad(const void* dy, const void* Wt, void* dx, int G, int NIg, int H, int Wd, int C, int R, int Ho,
                         int Wo, int N, int64_t sdy, int64_t sW, int64_t sdx, int dtype, hipStream_t s) {
  CMX_REQUIRE(G > 0 && NIg > 0 && C % 8 == 0 && R > 0 && Ho == H / R && Wo == Wd / R && Ho > 0 && Wo > 0, CMX_ERR_SHAPE,
              "conv_patch_dgrad: H=%d W=%d R=%d Ho=%d Wo=%d C=%d", H, Wd, R, Ho, Wo, C);
  const int M = NIg * Ho * Wo, Kc = R * R * C;
  GemmProblem p;
  p.A = dy; p.B = Wt; p.C = dx; p.G = G; p.M = M; p.N = Kc; p.K = N; p.lda = N; p.ldb = Kc; p.ldc = Kc;
  p.sA = sdy; p.sB = sW; p.sC = sdx; p.transB = 1; p.splitk = 1; p.dtype = dtype;
  p.scR = R; p.scH = H; p.scW = Wd; p.scC = C; p.scHo = Ho; p.scWo = Wo;
  return gemm_impl(p, s);
}

// DecoderHead.linear_fuse on the restructured decoder (MLPDecoder.py:66-77):
//   Z = e1 @ Wf[:, 3E:4E]^T + bias + up(z4) + up(z3) + up(z2)
// where z_i = e_i @ Wf[:, slot_i]^T are the low-resolution products of the upsampled branches
// (bilinear interpolation is linear with weights summing to 1, so it commutes with the 1x1
// conv: W up(e) = up(W e)).  e1 (B*H1*W1, K) row stride lda, z_i (B, h_i, w_i, E), Wf_c1 (E, K)
// row stride ldw: the c1 slice of the conv (K = E, DecoderFuseF) or, with linear_c1 folded in,
// the composed M_1 = Wf_c1 Wc_1 (K = C1, e1 = the stage-1 features; decoder_fold.hip).
// Z (B*H1*W1, E).  The (B, N1, 4E) concat of the reference is never formed.
int cmx_decoder_fuse_fwd(const void* e1, const void* Wf_c1, void* Z, const float* bias, const void* z4, const void* z3,
                         const void* z2, int B, int H1, int W1, int h4, int w4, int h3, int w3, int h2, int w2, int E,
                         int K, int64_t lda, int64_t ldw, int dtype, hipStream_t s) {
  CMX_REQUIRE(B > 0 && H1 > 0 && W1 > 0 && E > 0 && E % 8 == 0 && K > 0 && lda >= K && ldw >= K, CMX_ERR_SHAPE,
              "decoder_fuse_fwd: B=%d E=%d K=%d", B, E, K);
  UpSpec up{};
  const void* src[3] = {z4, z3, z2};
  const int hh[3] = {h4, h3, h2}, ww[3] = {w4, w3, w2};
  for (int q = 0; q < 3; ++q) {
    if (!src[q]) continue;
    up.src[up.n] = src[q]; up.h[up.n] = hh[q]; up.w[up.n] = ww[q]; ++up.n;
  }
  up.oH = H1; up.oW = W1;
  const int M = B * H1 * W1;
  GemmProblem p;
  p.A = e1; p.B = Wf_c1; p.C = Z; p.bias = bias; p.G = 1; p.M = M; p.N = E; p.K = K; p.lda = lda; p.ldb = ldw;
  p.ldc = E; p.splitk = 1; p.dtype = dtype; p.up = &up;
  return gemm_impl(p, s);
}


// ---------------------------------------------------------------- grouped (deferred) launches
size_t cmx_gemm_group_record_size(void) { return sizeof(GroupRec); }

// split for a problem inside a grouped launch: the launch is filled by many problems, so a
// split only bounds the k-loop of one block (<= 48 k-tiles of 64 = 3072 tokens per block)
int cmx_gemm_grouped_splitk(int G, int M, int N, int K, int ones_col) {
  if (G <= 0 || M <= 0 || N <= 0 || K <= 0) return 1;
  return gp::grouped_split(K, gemm_knobs());
}

int cmx_gemm_group_pack(void* rec, const void* A, const void* B, void* C, float* dbias, float* workspace, int G, int M,
                        int N, int K, int64_t lda, int64_t ldb, int64_t ldc, int64_t sA, int64_t sB, int64_t sC,
                        int64_t sdb, int transA, int transB, int out_mode, int ones_col, int splitk, int blk0) {
  CMX_REQUIRE(rec && G > 0 && M > 0 && N > 0 && K > 0 && blk0 >= 0, CMX_ERR_SHAPE, "gemm_group_pack: bad problem");
  CMX_REQUIRE(transA && transB, CMX_ERR_ARG, "gemm_group_pack: grouped launches take transA = transB = 1 (weight gradients)");
  CMX_REQUIRE(out_mode == 1 || out_mode == 2, CMX_ERR_ARG, "gemm_group_pack: fp32 output only");
  CMX_REQUIRE(!ones_col || (dbias && N >= 2), CMX_ERR_ARG, "gemm_group_pack: ones_col needs dbias");
  CMX_REQUIRE((long)M * N < (1L << 31), CMX_ERR_SHAPE, "gemm_group_pack: problem too large");
  CMX_REQUIRE(fast_ok(A, nullptr, B, M, N, K, K, lda, 0, ldb, sA, 0, sB, transA, transB, ones_col), CMX_ERR_ARG,
              "gemm_group_pack: operands not eligible for the bf16 LDS-DMA path");
  const int nb = ones_col ? N - 1 : N;
  const gp::GemmLaunch L = gp::plan_grouped(G, M, nb, K, splitk, gemm_knobs());
  CMX_REQUIRE((splitk > 0 ? splitk : L.nsplit) == 1 || workspace, CMX_ERR_ARG, "gemm_group_pack: split-K needs a workspace");
  GroupRec r{};
  GemmArgs& a = r.a;
  a.A = A; a.A2 = nullptr; a.B = B; a.C = C; a.dbias = dbias; a.ws = workspace;
  a.G = G; a.M = M; a.N = N; a.K = K; a.K1 = K; a.rows_per_sample = 1;
  a.act = 0; a.out_mode = out_mode; a.ones_col = ones_col; a.vec = 1;
  a.cvec = ((uintptr_t)C % 16 == 0) && (ldc * 4) % 16 == 0 && (sC * 4) % 16 == 0;
  a.lda = lda; a.ldb = ldb; a.ldc = ldc; a.sA = sA; a.sB = sB; a.sC = sC; a.sdb = sdb;
  set_plan(a, L);
  r.bm = L.bm; r.bn = L.bn;
  r.blk0 = blk0;
  r.nblk = (int)L.grid_x;
  memcpy(rec, &r, sizeof(r));
  return r.nblk;
}

// weight gradient of ONE tap of an NHWC convolution as a grouped-GEMM record:
// dW[g][n][tap*C + c] (row pitch K = KH*KW*C) = sum_m dy[g][m][n] * x[g][pixel(m) at tap][c]
int cmx_gemm_group_pack_conv_wgrad(void* rec, const void* dy, const void* x, float* dW, float* dbias, float* workspace,
                                   int G, int NIg, int H, int Wd, int C, int KH, int KW, int stride, int pad, int Ho,
                                   int Wo, int N, int tap, int64_t sdy, int64_t sx, int64_t sdW, int64_t sdb,
                                   int splitk, int blk0) {
  const int M = NIg * Ho * Wo;                  // reduction length (output pixels)
  CMX_REQUIRE(rec && G > 0 && N > 0 && C % 8 == 0 && N % 8 == 0 && M % 8 == 0 && tap >= 0 && tap < KH * KW,
              CMX_ERR_SHAPE, "gemm_group_pack_conv_wgrad: bad problem");
  CMX_REQUIRE(((uintptr_t)dy & 15) == 0 && ((uintptr_t)x & 15) == 0 && sdy % 8 == 0 && sx % 8 == 0, CMX_ERR_ARG,
              "gemm_group_pack_conv_wgrad: alignment");
  CMX_REQUIRE((long)NIg * H * Wd * C < (1L << 30) && (long)M * N < (1L << 30), CMX_ERR_SHAPE,
              "gemm_group_pack_conv_wgrad: too large for 31-bit offsets");
  const int ones = dbias ? 1 : 0;
  const int Nk = C + ones;                      // output columns (+ bias-gradient column)
  const gp::GemmLaunch L = gp::plan_grouped(G, N, C, M, splitk, gemm_knobs());
  CMX_REQUIRE((splitk > 0 ? splitk : L.nsplit) == 1 || workspace, CMX_ERR_ARG,
              "gemm_group_pack_conv_wgrad: split-K needs a workspace");
  GroupRec r{};
  GemmArgs& a = r.a;
  a.A = dy; a.B = x; a.C = dW + (long)tap * C; a.dbias = dbias; a.ws = workspace;
  a.G = G; a.M = N; a.N = Nk; a.K = M; a.K1 = M; a.rows_per_sample = 1;
  a.out_mode = 1; a.ones_col = ones; a.vec = 1;
  a.lda = N; a.sA = sdy; a.ldb = 0; a.sB = sx; a.ldc = (long)KH * KW * C; a.sC = sdW; a.sdb = sdb;
  a.cvec = (((uintptr_t)a.C % 16) == 0) && (a.ldc * 4) % 16 == 0 && (sdW * 4) % 16 == 0;
  a.conv = 2; a.cH = H; a.cW = Wd; a.cC = C; a.cKW = KW; a.cst = stride; a.cpad = pad; a.cHo = Ho; a.cWo = Wo;
  a.ctap = tap;
  set_plan(a, L);
  r.bm = L.bm; r.bn = L.bn;
  r.blk0 = blk0;
  r.nblk = (int)L.grid_x;
  memcpy(rec, &r, sizeof(r));
  return r.nblk;
}

// y[g] (NIg*Ho*Wo, N) = conv(x[g]) + bias[g] with the im2col done by the GEMM's operand DMA
// (OverlapPatchEmbed.proj k3 s2 p1, dual_segformer.py:196-197; Attention.sr kR sR, :95-96).
// bf16, NHWC x with C % 64 == 0, weights (N, KH, KW, C).
int cmx_conv_implicit_fwd(const void* x, const void* Wt, void* y, const float* bias, float* workspace, int G, int NIg,
                          int H, int Wd, int C, int KH, int KW, int stride, int pad, int Ho, int Wo, int N, int64_t sx,
                          int64_t sW, int64_t sy, int64_t sbias, int splitk, int dtype, hipStream_t s) {
  CMX_REQUIRE((dtype == 1 || dtype == 2) && C % 64 == 0 && N % 8 == 0 && G > 0 && NIg > 0, CMX_ERR_SHAPE,
              "conv_implicit_fwd: bf16 / fp16 with C %% 64 == 0 only (C=%d, N=%d)", C, N);
  CMX_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)Wt & 15) == 0 && ((uintptr_t)y & 15) == 0 && sx % 8 == 0 &&
              sW % 8 == 0 && sy % 8 == 0, CMX_ERR_ARG, "conv_implicit_fwd: alignment");
  const long M = (long)NIg * Ho * Wo, K = (long)KH * KW * C;
  CMX_REQUIRE((long)NIg * H * Wd * C < (1L << 30) && M * N < (1L << 31) && (long)N * K < (1L << 30), CMX_ERR_SHAPE,
              "conv_implicit_fwd: too large for 31-bit offsets");
  GemmArgs a{};
  a.A = x; a.B = Wt; a.C = y; a.bias = bias;
  a.G = G; a.M = (int)M; a.N = N; a.K = (int)K; a.K1 = (int)K; a.rows_per_sample = 1; a.vec = 1;
  a.lda = 0; a.sA = sx; a.ldb = K; a.sB = sW; a.ldc = N; a.sC = sy; a.sbias = sbias;
  a.cvec = (N * 2) % 16 == 0 && (sy * 2) % 16 == 0;
  a.conv = 1; a.cH = H; a.cW = Wd; a.cC = C; a.cKW = KW; a.cst = stride; a.cpad = pad; a.cHo = Ho; a.cWo = Wo;
  // the SR conv has few output pixels and a long K (stage 1: 600 x 64 x 4096): split K like a
  // plain GEMM (splitk <= 0: the library's choice, cmx_gemm_splitk(G, M, N, K, 0, 1))
  gp::GemmShape shape;
  shape.G = G; shape.M = (int)M; shape.N = N; shape.K = (int)K; shape.dtype = dtype; shape.fast = 1;
  shape.splitk = splitk; shape.tile_only = 1;
  const gp::GemmLaunch L = gp::plan_gemm(shape, gemm_knobs(), cu_count());
  CMX_REQUIRE((splitk > 0 ? splitk : L.nsplit) == 1 || workspace, CMX_ERR_ARG, "conv_implicit_fwd: split-K needs a workspace");
  a.ws = workspace;
  set_plan(a, L);
  const int st = launch_gemm(L, a, 0, 0, dtype, s);
  return st != CMX_OK ? st : cmx_check_launch("conv_implicit_fwd");
}

int cmx_gemm_grouped(const void* recs, int nrec, int total_blocks, int dtype, hipStream_t s) {
  CMX_REQUIRE(dtype == 1 || dtype == 2, CMX_ERR_DTYPE, "gemm_grouped: operands bf16 (1) or fp16 (2), got %d", dtype);
  CMX_REQUIRE(recs && nrec > 0 && total_blocks > 0, CMX_ERR_ARG, "gemm_grouped: empty launch");
  // XCD map of the grouped grid: chunked round-robin with 64-tile runs (CMX_GROUPED_CHUNK=n to
  // change the run, 0 = the contiguous xcd_tile map).  Measured on the B2 step's 8174-block
  // launch: 695-702 us contiguous, 624-633 us for runs of 4..128 tiles
  // (scripts/grouped_chunk_sweep.sh); PMC HBM bytes per launch 3.13 GB at 16-tile runs,
  // 2.48 GB at 64 (contiguous: 2.43 GB), so 64 keeps the L2 reuse of neighbouring tiles
  return cmx_gemm_grouped_capped(recs, nrec, total_blocks, 0, dtype, s);
}

int cmx_gemm_grouped_capped(const void* recs, int nrec, int total_blocks, int max_blocks, int dtype, hipStream_t s) {
  CMX_REQUIRE(dtype == 1 || dtype == 2, CMX_ERR_DTYPE, "gemm_grouped: operands bf16 (1) or fp16 (2), got %d", dtype);
  CMX_REQUIRE(recs && nrec > 0 && total_blocks > 0, CMX_ERR_ARG, "gemm_grouped: empty launch");
  CMX_REQUIRE(max_blocks <= 0 || max_blocks % 8 == 0, CMX_ERR_ARG, "gemm_grouped: max_blocks %d not a multiple of 8",
              max_blocks);
  static int& chunk = cmx_knob("GROUPED_CHUNK", 64);
  const GroupRec* rr = (const GroupRec*)recs;
  const int grid = max_blocks > 0 && max_blocks < total_blocks ? max_blocks : total_blocks;
  if (grid < total_blocks) {
    if (dtype == 2)
      hipLaunchKernelGGL((gemm_grouped_kernel<f16, 2, true>), dim3(grid), dim3(256), 0, s, rr, nrec, chunk, total_blocks);
    else
      hipLaunchKernelGGL((gemm_grouped_kernel<bf16, 2, true>), dim3(grid), dim3(256), 0, s, rr, nrec, chunk, total_blocks);
  } else if (dtype == 2) {
    hipLaunchKernelGGL((gemm_grouped_kernel<f16>), dim3(grid), dim3(256), 0, s, rr, nrec, chunk, total_blocks);
  } else {
    hipLaunchKernelGGL((gemm_grouped_kernel<bf16>), dim3(grid), dim3(256), 0, s, rr, nrec, chunk, total_blocks);
  }
  return cmx_check_launch("gemm_grouped");
}

size_t cmx_reduce_record_size(void) { return sizeof(RedRec); }

int cmx_reduce_pack(void* rec, const float* src, float* dst, float* dst2, int G, int nblk, int64_t sg, int64_t sb,
                    int rows, int cols, int csplit, int64_t dg, int ldd, int64_t dg2, int ldd2, int accumulate,
                    int blk0) {
  CMX_REQUIRE(rec && src && dst && G > 0 && nblk > 0 && rows > 0 && cols > 0 && blk0 >= 0, CMX_ERR_SHAPE,
              "reduce_pack: bad reduction");
  CMX_REQUIRE(csplit >= cols || (dst2 && csplit >= 0), CMX_ERR_ARG, "reduce_pack: columns past csplit need dst2");
  RedRec r{};
  r.src = src; r.dst = dst; r.dst2 = dst2; r.sg = sg; r.sb = sb; r.dg = dg; r.dg2 = dg2;
  r.ldd = ldd; r.ldd2 = ldd2; r.G = G; r.nblk = nblk; r.rows = rows; r.cols = cols; r.csplit = csplit;
  r.accumulate = accumulate;
  r.zl = nblk <= 8 ? 1 : (nblk <= 64 ? 4 : 16);
  r.cpg = (int)cdiv((long)rows * cols, 256 / r.zl);
  r.blk0 = blk0;
  memcpy(rec, &r, sizeof(r));
  return r.cpg * G;
}

int cmx_reduce_grouped(const void* recs, int nrec, int total_blocks, hipStream_t s) {
  CMX_REQUIRE(recs && nrec > 0 && total_blocks > 0, CMX_ERR_ARG, "reduce_grouped: empty launch");
  hipLaunchKernelGGL(reduce_grouped_kernel, dim3(total_blocks), dim3(256), 0, s, (const RedRec*)recs, nrec);
  return cmx_check_launch("reduce_grouped");
}

}  // extern "C"
