// ASPP's dilated 3x3 convolutions of the DeepLabV3+ head (deeplabv3plus.py:37-47, :78-80): Cin -> Cout with both a
// multiple of 64, three rates, ONE shared input (the stage-4 map, 15 x 20 at 480 x 640).  The structure is
// easpp.hip's, widened: one wave per 32 pixels x 64 channels on 32x32 MFMA tiles, both operands read straight from
// global memory (the map and the live taps' weights sit in L2), no im2col buffer, a tap that leaves the map for every
// pixel skipped by the whole grid (15 x 20, rates 12 / 24 / 36: 11 of the 27 taps are live).
//
//   aspp_fwd_kernel<T>:   y_g = conv(x, w_g); blockIdx = (32-pixel tile, 64 output channels, branch).
//   aspp_dgrad_kernel<T>: dx = sum_g conv^T(dy_g, w_g): the three branches read the same x, so their input gradients
//     are summed in the accumulator and rounded once; blockIdx = (32-pixel tile, 64 input channels).
//   aspp_wgrad_kernel<T>: dW_g[co][tap][ci] = sum_p dY_g[p][co] X[p + off][ci]; blockIdx = (row chunk x 64x64 slice,
//     tap, branch), both operands gathered along the pixel axis.  Per-chunk fp32 partials, folded in chunk order by
//     aspp_fold3_kernel (one chunk: written in place).
// Sums are kept short: a tap's (or a 128-row block's) products are summed on their own and then added, so the fp32
// rounding grows with the chain's length, not with 9 Cin.  No atomics on floats: bit-identical from run to run.
#include "cmx_mfma.h"
#include "../../include/cmx_deeplab.h"  // compiler-checks the definitions below against the ABI header

namespace {

constexpr int TAPS = 9;
constexpr int CT = 64;                    // channels per wave, both sides
constexpr int CMAX = 1024;
constexpr int SUB_ROWS = 128;             // rows of the weight gradient summed on their own before they are added
constexpr int MAX_CHUNKS = 8;

struct Aspp3 {                            // a: the pixel-side inputs (fwd: a[0] = x alone), w: weights (wgrad: w[0] =
  const void* a[3];                       // x alone), o: outputs (dgrad: o[0] = dx alone)
  const void* w[3];
  void* o[3];
  int rate[3];
};

template <typename T>
__global__ __launch_bounds__(64) void aspp_fwd_kernel(Aspp3 P, int B, int h, int w, int Cin, long ldx, long ldy) {
  constexpr int V = KV<T>, STEP = 2 * V;
  const int g = blockIdx.z, cb = blockIdx.y * CT;
  const T* __restrict__ x = (const T*)P.a[0];
  const T* __restrict__ wt = (const T*)P.w[g];
  T* __restrict__ y = (T*)P.o[g];
  const int rate = P.rate[g];
  const long M = (long)B * h * w;
  const int r = threadIdx.x & 31, hh = threadIdx.x >> 5;
  const long pix = (long)blockIdx.x * 32 + r;
  const bool pok = pix < M;
  const int rem = (int)((pok ? pix : 0) % ((long)h * w));
  const int py = rem / w, px = rem % w;
  f32x16 acc0 = zero16(), acc1 = zero16();
  for (int ky = 0; ky < 3; ++ky) {
    const int dy = (ky - 1) * rate;
    if (dy <= -h || dy >= h) continue;             // the tap leaves the map for every pixel (block-uniform)
    for (int kx = 0; kx < 3; ++kx) {
      const int dx = (kx - 1) * rate;
      if (dx <= -w || dx >= w) continue;
      const int tap = ky * 3 + kx;
      const int yy = py + dy, xx = px + dx;
      const bool ok = pok && yy >= 0 && yy < h && xx >= 0 && xx < w;      // zero padding
      const T* arow = x + (ok ? pix + (long)dy * w + dx : 0) * ldx + V * hh;
      const T* w0 = wt + ((long)(cb + r) * TAPS + tap) * Cin + V * hh;     // A[c = co][k = ci]: contiguous in k
      const T* w1 = w0 + (long)32 * TAPS * Cin;
      f32x16 t0 = zero16(), t1 = zero16();
      for (int k = 0; k < Cin; k += STEP) {
        Raw<T> bv = load_raw<T>(arow + k);
        if (!ok) bv = zero_raw<T>();
        t0 = mma_step<T>(load_raw<T>(w0 + k), bv, t0);
        t1 = mma_step<T>(load_raw<T>(w1 + k), bv, t1);
      }
      acc0 += t0;
      acc1 += t1;
    }
  }
  if (pok) {
    store_acc_row<T>(y + pix * ldy + cb, acc0, 0, hh, 1.f);
    store_acc_row<T>(y + pix * ldy + cb, acc1, 1, hh, 1.f);
  }
}

// a = dy_g, o[0] = dx; taps mirrored, w read as (ci, co): k strides over the weight's rows
template <typename T>
__global__ __launch_bounds__(64) void aspp_dgrad_kernel(Aspp3 P, int B, int h, int w, int Cin, int Cout, long lddy,
                                                  long lddx) {
  constexpr int V = KV<T>, STEP = 2 * V;
  const int cb = blockIdx.y * CT;
  T* __restrict__ o = (T*)P.o[0];
  const long M = (long)B * h * w;
  const int r = threadIdx.x & 31, hh = threadIdx.x >> 5;
  const long pix = (long)blockIdx.x * 32 + r;
  const bool pok = pix < M;
  const int rem = (int)((pok ? pix : 0) % ((long)h * w));
  const int py = rem / w, px = rem % w;
  const long wrow = (long)TAPS * Cin;              // elements between two output channels of one tap
  f32x16 acc0 = zero16(), acc1 = zero16();
  for (int g = 0; g < 3; ++g) {
    const T* __restrict__ a = (const T*)P.a[g];
    const T* __restrict__ wt = (const T*)P.w[g];
    const int rate = -P.rate[g];
    for (int ky = 0; ky < 3; ++ky) {
      const int dy = (ky - 1) * rate;
      if (dy <= -h || dy >= h) continue;
      for (int kx = 0; kx < 3; ++kx) {
        const int dx = (kx - 1) * rate;
        if (dx <= -w || dx >= w) continue;
        const int tap = ky * 3 + kx;
        const int yy = py + dy, xx = px + dx;
        const bool ok = pok && yy >= 0 && yy < h && xx >= 0 && xx < w;
        const T* arow = a + (ok ? pix + (long)dy * w + dx : 0) * lddy + V * hh;
        const T* wk = wt + (long)(V * hh) * wrow + (long)tap * Cin + cb + r;      // A[c = ci][k = co]
        f32x16 t0 = zero16(), t1 = zero16();
        for (int k = 0; k < Cout; k += STEP) {
          Raw<T> bv = load_raw<T>(arow + k);
          if (!ok) bv = zero_raw<T>();
          T e0[V], e1[V];
#pragma unroll
          for (int j = 0; j < V; ++j) {
            const T* p = wk + (long)(k + j) * wrow;
            e0[j] = p[0];
            e1[j] = p[32];
          }
          t0 = mma_step<T>(pack_raw<T>(e0), bv, t0);
          t1 = mma_step<T>(pack_raw<T>(e1), bv, t1);
        }
        acc0 += t0;
        acc1 += t1;
      }
    }
  }
  if (pok) {
    store_acc_row<T>(o + pix * lddx + cb, acc0, 0, hh, 1.f);
    store_acc_row<T>(o + pix * lddx + cb, acc1, 1, hh, 1.f);
  }
}

// a = dy_g, w[0] = x, o = dw_g (fp32); blockIdx = (chunk * ntile + (co tile * Cin/64 + ci tile), tap, branch)
template <typename T>
__global__ __launch_bounds__(64) void aspp_wgrad_kernel(Aspp3 P, float* __restrict__ ws, int nchunk, int rows, int B, int h,
                                                  int w, int Cin, int Cout, long lddy, long ldx) {
  constexpr int V = KV<T>, STEP = 2 * V;
  const int nci = Cin / CT, ntile = nci * (Cout / CT);
  const int g = blockIdx.z, tap = blockIdx.y, chunk = blockIdx.x / ntile, tile = blockIdx.x % ntile;
  const int cob = (tile / nci) * CT, cib = (tile % nci) * CT;
  const long wsz = (long)Cout * TAPS * Cin;
  const T* __restrict__ dy = (const T*)P.a[g] + cob;
  const T* __restrict__ x = (const T*)P.w[0] + cib;
  float* __restrict__ dst = nchunk == 1 ? (float*)P.o[g] : ws + ((long)g * nchunk + chunk) * wsz;
  const int rate = P.rate[g];
  const int oy = (tap / 3 - 1) * rate, ox = (tap % 3 - 1) * rate;
  const long M = (long)B * h * w;
  const long kbeg = (long)chunk * rows;
  const long kend = kbeg + rows < M ? kbeg + rows : M;
  const int r = threadIdx.x & 31, hh = threadIdx.x >> 5;
  f32x16 acc[2][2] = {{zero16(), zero16()}, {zero16(), zero16()}};      // [co tile][ci tile]
  const bool skip = oy <= -h || oy >= h || ox <= -w || ox >= w;        // its slice of dW is zero
  if (!skip) {
    for (long s0 = kbeg; s0 < kend; s0 += SUB_ROWS) {
      const long send = s0 + SUB_ROWS < kend ? s0 + SUB_ROWS : kend;
      f32x16 t[2][2] = {{zero16(), zero16()}, {zero16(), zero16()}};
      for (long k0 = s0; k0 < send; k0 += STEP) {
        // this lane half's V pixels k0 + V hh + j: (py, px) of the first by division, the rest by stepping
        const long p0 = k0 + V * hh;
        const int rem = (int)(p0 % ((long)h * w));
        int py = rem / w, px = rem % w;
        T ea[2][V], eb[2][V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const long p = p0 + j;
          const bool pok = p < send;
          const int yy = py + oy, xx = px + ox;
          const bool ok = pok && yy >= 0 && yy < h && xx >= 0 && xx < w;
          const T* pa = dy + (pok ? p : 0) * lddy + r;
          const T* pb = x + (ok ? p + (long)oy * w + ox : 0) * ldx + r;
          ea[0][j] = pok ? pa[0] : T{};
          ea[1][j] = pok ? pa[32] : T{};
          eb[0][j] = ok ? pb[0] : T{};
          eb[1][j] = ok ? pb[32] : T{};
          if (++px == w) { px = 0; if (++py == h) py = 0; }
        }
        const Raw<T> a0 = pack_raw<T>(ea[0]), a1 = pack_raw<T>(ea[1]);
        const Raw<T> b0 = pack_raw<T>(eb[0]), b1 = pack_raw<T>(eb[1]);
        t[0][0] = mma_step<T>(a0, b0, t[0][0]);
        t[0][1] = mma_step<T>(a0, b1, t[0][1]);
        t[1][0] = mma_step<T>(a1, b0, t[1][0]);
        t[1][1] = mma_step<T>(a1, b1, t[1][1]);
      }
      acc[0][0] += t[0][0];
      acc[0][1] += t[0][1];
      acc[1][0] += t[1][0];
      acc[1][1] += t[1][1];
    }
  }
#pragma unroll
  for (int tc = 0; tc < 2; ++tc)
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int co = cob + 32 * tc + accrow(i, hh);
        dst[((long)co * TAPS + tap) * Cin + cib + 32 * ti + r] = acc[tc][ti][i];
      }
}

// o_g[i] = sum over the chunks, in order, of ws[g][chunk][i]
__global__ __launch_bounds__(256) void aspp_fold3_kernel(const float* __restrict__ ws, float* o0, float* o1, float* o2,
                                                   int nchunk, long wsz) {
  const int g = blockIdx.y;
  const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= wsz) return;
  float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int c = 0; c < nchunk; ++c) {
    const float4 v = *reinterpret_cast<const float4*>(ws + ((long)g * nchunk + c) * wsz + i);
    t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w;
  }
  float* o = g == 0 ? o0 : g == 1 ? o1 : o2;
  *reinterpret_cast<float4*>(o + i) = t;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
bool chan_ok(int C) { return C >= CT && C <= CMAX && C % CT == 0; }
bool shape_ok(int B, int h, int w, int Cin, int Cout) {
  return B > 0 && h > 0 && w > 0 && (long)B * h * w < (1L << 31) - 64 && chan_ok(Cin) && chan_ok(Cout);
}

// the checks the three entry points share.  a: the na pixel-side inputs of ca channels (stride lda), b: the nb
// second operands (weights, or x with stride ldb >= cb when ldb > 0), o: the no outputs (stride ldo when ldo > 0)
int check(const char* what, const void* const* a, int na, const void* const* b, int nb, const void* const* o, int no,
          int B, int h, int w, int Cin, int Cout, const int* rate, long lda, int ca, long ldb, int cb, long ldo, int co,
          int dtype) {
  CMX_REQUIRE(dtype >= 0 && dtype <= 2, CMX_ERR_DTYPE, "%s: unsupported dtype %d", what, dtype);
  CMX_REQUIRE(shape_ok(B, h, w, Cin, Cout), CMX_ERR_SHAPE,
              "%s: B=%d h=%d w=%d Cin=%d Cout=%d (channels: multiples of %d up to %d)", what, B, h, w, Cin, Cout, CT, CMAX);
  const int V = dtype == 0 ? 4 : 8;
  for (int i = 0; i < na; ++i) CMX_REQUIRE(a[i], CMX_ERR_ARG, "%s: null operand", what);
  for (int i = 0; i < nb; ++i) CMX_REQUIRE(b[i], CMX_ERR_ARG, "%s: null operand", what);
  for (int i = 0; i < no; ++i) CMX_REQUIRE(o[i], CMX_ERR_ARG, "%s: null operand", what);
  for (int i = 0; i < na; ++i) CMX_REQUIRE(aligned16(a[i]), CMX_ERR_ARG, "%s: an operand off a 16-byte boundary", what);
  for (int i = 0; i < nb; ++i) CMX_REQUIRE(aligned16(b[i]), CMX_ERR_ARG, "%s: an operand off a 16-byte boundary", what);
  for (int i = 0; i < no; ++i) CMX_REQUIRE(aligned16(o[i]), CMX_ERR_ARG, "%s: an operand off a 16-byte boundary", what);
  for (int g = 0; g < 3; ++g) CMX_REQUIRE(rate[g] >= 1, CMX_ERR_ARG, "%s: rate %d of branch %d", what, rate[g], g);
  CMX_REQUIRE(lda >= ca && lda % V == 0 && (ldb == 0 || (ldb >= cb && ldb % V == 0)) &&
              (ldo == 0 || (ldo >= co && ldo % V == 0)), CMX_ERR_ARG,
              "%s: row strides %ld / %ld / %ld (at least the row's channels, multiples of %d)", what, lda, ldb, ldo, V);
  return CMX_OK;
}

// rows per chunk of the weight gradient: a multiple of SUB_ROWS, grown with the number of 64 x 64 slices (which give
// the launch its width already) so that the partials stay a small multiple of the result, and at most MAX_CHUNKS
long wg_rows(long M, int Cin, int Cout) {
  const int ntile = (Cin / CT) * (Cout / CT);
  long rows = (long)SUB_ROWS * (ntile < 16 ? ntile : 16);
  const long least = ((M + MAX_CHUNKS - 1) / MAX_CHUNKS + SUB_ROWS - 1) / SUB_ROWS * SUB_ROWS;
  return rows > least ? rows : least;
}

}  // namespace

extern "C" {

int cmx_aspp_conv_fwd(const void* x, const void* w0, const void* w1, const void* w2, void* y0, void* y1, void* y2, int B,
                      int h, int w, int Cin, int Cout, int r0, int r1, int r2, int64_t ldx, int64_t ldy, int dtype,
                      hipStream_t s) {
  const void* a[1] = {x};
  const void* wt[3] = {w0, w1, w2};
  const void* o[3] = {y0, y1, y2};
  const int rate[3] = {r0, r1, r2};
  const int st = check("aspp_conv_fwd", a, 1, wt, 3, o, 3, B, h, w, Cin, Cout, rate, (long)ldx, Cin, 0, 0, (long)ldy,
                       Cout, dtype);
  if (st != CMX_OK) return st;
  Aspp3 P = {};
  P.a[0] = x;
  for (int g = 0; g < 3; ++g) { P.w[g] = wt[g]; P.o[g] = (void*)o[g]; P.rate[g] = rate[g]; }
  const dim3 grid(cdiv((long)B * h * w, 32), Cout / CT, 3);
  CMX_DISPATCH(dtype, T, {
    hipLaunchKernelGGL(aspp_fwd_kernel<T>, grid, dim3(64), 0, s, P, B, h, w, Cin, (long)ldx, (long)ldy);
  });
  return cmx_check_launch("aspp_conv_fwd");
}

int cmx_aspp_conv_dgrad(const void* dy0, const void* dy1, const void* dy2, const void* w0, const void* w1, const void* w2,
                        void* dx, int B, int h, int w, int Cin, int Cout, int r0, int r1, int r2, int64_t lddy,
                        int64_t lddx, int dtype, hipStream_t s) {
  const void* a[3] = {dy0, dy1, dy2};
  const void* wt[3] = {w0, w1, w2};
  const void* o[1] = {dx};
  const int rate[3] = {r0, r1, r2};
  const int st = check("aspp_conv_dgrad", a, 3, wt, 3, o, 1, B, h, w, Cin, Cout, rate, (long)lddy, Cout, 0, 0,
                       (long)lddx, Cin, dtype);
  if (st != CMX_OK) return st;
  Aspp3 P = {};
  P.o[0] = dx;
  for (int g = 0; g < 3; ++g) { P.a[g] = a[g]; P.w[g] = wt[g]; P.rate[g] = rate[g]; }
  const dim3 grid(cdiv((long)B * h * w, 32), Cin / CT);
  CMX_DISPATCH(dtype, T, {
    hipLaunchKernelGGL(aspp_dgrad_kernel<T>, grid, dim3(64), 0, s, P, B, h, w, Cin, Cout, (long)lddy, (long)lddx);
  });
  return cmx_check_launch("aspp_conv_dgrad");
}

size_t cmx_aspp_conv_wgrad_workspace(int B, int h, int w, int Cin, int Cout) {
  if (!shape_ok(B, h, w, Cin, Cout)) return 0;
  const long M = (long)B * h * w;
  const long nc = (M + wg_rows(M, Cin, Cout) - 1) / wg_rows(M, Cin, Cout);
  return nc > 1 ? (size_t)3 * nc * Cout * TAPS * Cin * sizeof(float) : 0;
}

int cmx_aspp_conv_wgrad(const void* dy0, const void* dy1, const void* dy2, const void* x, float* dw0, float* dw1,
                        float* dw2, float* workspace, int B, int h, int w, int Cin, int Cout, int r0, int r1, int r2,
                        int64_t lddy, int64_t ldx, int dtype, hipStream_t s) {
  const void* a[3] = {dy0, dy1, dy2};
  const void* xs[1] = {x};
  const void* o[3] = {dw0, dw1, dw2};
  const int rate[3] = {r0, r1, r2};
  int st = check("aspp_conv_wgrad", a, 3, xs, 1, o, 3, B, h, w, Cin, Cout, rate, (long)lddy, Cout, (long)ldx, Cin, 0, 0,
                 dtype);
  if (st != CMX_OK) return st;
  const long M = (long)B * h * w;
  const long rows = wg_rows(M, Cin, Cout);
  const int nc = (int)((M + rows - 1) / rows);
  CMX_REQUIRE(nc == 1 || (workspace && aligned16(workspace)), CMX_ERR_ARG, "aspp_conv_wgrad: null workspace");
  Aspp3 P = {};
  P.w[0] = x;
  for (int g = 0; g < 3; ++g) { P.a[g] = a[g]; P.o[g] = (void*)o[g]; P.rate[g] = rate[g]; }
  const int ntile = (Cin / CT) * (Cout / CT);
  CMX_DISPATCH(dtype, T, {
    hipLaunchKernelGGL(aspp_wgrad_kernel<T>, dim3(nc * ntile, TAPS, 3), dim3(64), 0, s, P, workspace, nc, (int)rows, B, h, w,
                       Cin, Cout, (long)lddy, (long)ldx);
  });
  st = cmx_check_launch("aspp_conv_wgrad");
  if (st != CMX_OK || nc == 1) return st;
  const long wsz = (long)Cout * TAPS * Cin;
  hipLaunchKernelGGL(aspp_fold3_kernel, dim3(cdiv(wsz, 256 * 4), 3), dim3(256), 0, s, workspace, dw0, dw1, dw2, nc, wsz);
  return cmx_check_launch("aspp_conv_wgrad fold");
}

}  // extern "C"
