// The eASPP neck of the mit_b*_w_ef_aspp backbones (dual_segformer_w_ef_aspp.py:18-157) on the stage-4 fused map
// (15 x 20 at 480 x 640): what its 18 convolutions need beyond the GEMM family.
//
//   easpp_conv_kernel<T, DGRAD>: the dilated 3x3 64 -> 64 convolution of the three branches of one depth level as ONE
//     grid (blockIdx.y = branch), and its input gradient (the same convolution with mirrored taps and the weight
//     read transposed).  One wave per 32 pixels x 64 channels: D[c][pixel] += W_tap[c][k] * X[pixel + off(tap)][k]
//     on 32x32 MFMA tiles, both operands read straight from global memory (the map and one branch's nine taps live
//     in L2; nothing is staged, no im2col buffer exists).  A tap whose offset leaves the map for every pixel is
//     skipped by the whole grid: on 15 x 20, rate 12 keeps all nine, rates 24 and 36 keep the centre tap alone.
//   easpp_wgrad_kernel<T>: dW[co][tap][ci] = sum_p dY[p][co] X[p + off(tap)][ci]; blockIdx = (128-row chunk, tap, branch),
//     one wave per 64 x 64 tap slice, both operands gathered along the pixel axis.  Per-chunk fp32 partials,
//     folded in chunk order by easpp_fold3_kernel (one chunk: written in place).
//   concat / pooled-branch / dropout-mask kernels: see include/cmx_easpp.h.
// No atomics on floats anywhere: every result is bit-identical from run to run.
#include "cmx_mfma.h"
#include "../../include/cmx_easpp.h"  // compiler-checks the definitions below against the ABI header

namespace {

constexpr int CW = 64;                    // reduce_dim (:53): the branch width
constexpr int TAPS = 9;
constexpr int WSZ = CW * TAPS * CW;       // one branch's weight elements
constexpr int WG_ROWS = 128;              // rows per workgroup of the weight gradient

struct Group3 {                           // the three branches' operands: a = pixel-side input, w = weights /
  const void* a[3];                       // second input, o = output
  const void* w[3];
  void* o[3];
  int rate[3];
};

// forward: a = x, o = y;  DGRAD: a = dy, o = dx (taps mirrored, w read as (ci, co))
template <typename T, bool DGRAD>
__global__ __launch_bounds__(64) void easpp_conv_kernel(Group3 P, int B, int h, int w, long lda, long ldo) {
  constexpr int V = KV<T>, STEP = 2 * V;
  const int g = blockIdx.y;
  const T* __restrict__ a = (const T*)P.a[g];
  const T* __restrict__ wt = (const T*)P.w[g];
  T* __restrict__ o = (T*)P.o[g];
  const int rate = DGRAD ? -P.rate[g] : P.rate[g];
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
      const T* arow = a + (ok ? pix + (long)dy * w + dx : 0) * lda + V * hh;
      // each tap summed on its own, then added: the fp32 rounding grows with 64 + 9 terms, not 576
      f32x16 t0 = zero16(), t1 = zero16();
#pragma unroll
      for (int s = 0; s < CW / STEP; ++s) {
        const int k = s * STEP + V * hh;
        Raw<T> bv = load_raw<T>(arow + s * STEP);
        if (!ok) bv = zero_raw<T>();
        Raw<T> a0, a1;
        if constexpr (!DGRAD) {                    // A[c = co][k = ci]: contiguous in k
          a0 = load_raw<T>(wt + ((long)r * TAPS + tap) * CW + k);
          a1 = load_raw<T>(wt + ((long)(32 + r) * TAPS + tap) * CW + k);
        } else {                                   // A[c = ci][k = co]: k strides over the weight's rows
          T e0[V], e1[V];
#pragma unroll
          for (int j = 0; j < V; ++j) {
            const T* p = wt + ((long)(k + j) * TAPS + tap) * CW + r;
            e0[j] = p[0];
            e1[j] = p[32];
          }
          a0 = pack_raw<T>(e0);
          a1 = pack_raw<T>(e1);
        }
        t0 = mma_step<T>(a0, bv, t0);
        t1 = mma_step<T>(a1, bv, t1);
      }
      acc0 += t0;
      acc1 += t1;
    }
  }
  if (pok) {
    store_acc_row<T>(o + pix * ldo, acc0, 0, hh, 1.f);
    store_acc_row<T>(o + pix * ldo, acc1, 1, hh, 1.f);
  }
}

// a = dy, w = x, o = dw (fp32); blockIdx = (chunk, tap, branch)
template <typename T>
__global__ __launch_bounds__(64) void easpp_wgrad_kernel(Group3 P, float* __restrict__ ws, int nchunk, int B, int h, int w,
                                                   long lddy, long ldx) {
  constexpr int V = KV<T>, STEP = 2 * V;
  const int g = blockIdx.z, tap = blockIdx.y, chunk = blockIdx.x;
  const T* __restrict__ dy = (const T*)P.a[g];
  const T* __restrict__ x = (const T*)P.w[g];
  float* __restrict__ dst = nchunk == 1 ? (float*)P.o[g] : ws + ((long)g * nchunk + chunk) * WSZ;
  const int rate = P.rate[g];
  const int oy = (tap / 3 - 1) * rate, ox = (tap % 3 - 1) * rate;
  const long M = (long)B * h * w;
  const long kbeg = (long)chunk * WG_ROWS;
  const long kend = kbeg + WG_ROWS < M ? kbeg + WG_ROWS : M;
  const int r = threadIdx.x & 31, hh = threadIdx.x >> 5;
  f32x16 acc[2][2] = {{zero16(), zero16()}, {zero16(), zero16()}};      // [co tile][ci tile]
  const bool skip = oy <= -h || oy >= h || ox <= -w || ox >= w;        // its slice of dW is zero
  if (!skip) {
    for (long k0 = kbeg; k0 < kend; k0 += STEP) {
      // this lane half's V pixels k0 + V hh + j: (py, px) of the first by division, the rest by stepping
      const long p0 = k0 + V * hh;
      const int rem = (int)(p0 % ((long)h * w));
      int py = rem / w, px = rem % w;
      T ea[2][V], eb[2][V];
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const long p = p0 + j;
        const bool pok = p < kend;
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
      acc[0][0] = mma_step<T>(a0, b0, acc[0][0]);
      acc[0][1] = mma_step<T>(a0, b1, acc[0][1]);
      acc[1][0] = mma_step<T>(a1, b0, acc[1][0]);
      acc[1][1] = mma_step<T>(a1, b1, acc[1][1]);
    }
  }
#pragma unroll
  for (int tc = 0; tc < 2; ++tc)
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int co = 32 * tc + accrow(i, hh);
        dst[((long)co * TAPS + tap) * CW + 32 * ti + r] = acc[tc][ti][i];
      }
}

// o_g[i] = sum over the chunks, in order, of ws[g][chunk][i].  cmx_partials_sum folds (G, nblk, W) partials into ONE
// contiguous (G, W) output; the three branches' weights are separate parameters of the flat gradient buffer (their
// BatchNorms lie between), so it would take three launches per depth level where this takes one.
__global__ __launch_bounds__(256) void easpp_fold3_kernel(const float* __restrict__ ws, float* o0, float* o1, float* o2,
                                                    int nchunk) {
  const int g = blockIdx.y;
  const int i = (blockIdx.x * 256 + threadIdx.x) * 4;
  float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int c = 0; c < nchunk; ++c) {
    const float4 v = *reinterpret_cast<const float4*>(ws + ((long)g * nchunk + c) * WSZ + i);
    t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w;
  }
  float* o = g == 0 ? o0 : g == 1 ? o1 : o2;
  *reinterpret_cast<float4*>(o + i) = t;
}

// cat row = [y0 | y1 | y2 | y3 | pool[b]]: one 16-B vector per thread
template <typename T>
__global__ __launch_bounds__(256) void easpp_concat_fwd_kernel(const T* __restrict__ y0, const T* __restrict__ y1,
                                                         const T* __restrict__ y2, const T* __restrict__ y3,
                                                         const float* __restrict__ pool, T* __restrict__ cat, long M,
                                                         int N, int Cm) {
  constexpr int V = VecT<T>::N;
  const int vpr = 5 * Cm / V, vps = Cm / V;
  const long nvec = M * vpr;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (long)gridDim.x * 256) {
    const long row = i / vpr;
    const int cv = (int)(i % vpr), slot = cv / vps, c = (cv % vps) * V;
    T* dst = cat + row * 5 * Cm + (long)slot * Cm + c;
    if (slot < 4) {
      const T* src = slot == 0 ? y0 : slot == 1 ? y1 : slot == 2 ? y2 : y3;
      *reinterpret_cast<Raw<T>*>(dst) = load_raw<T>(src + row * Cm + c);
    } else {
      float v[V];
#pragma unroll
      for (int j = 0; j < V; ++j) v[j] = pool[(row / N) * Cm + c + j];
      store_vec<T>(dst, v);
    }
  }
}

// blocks [0, ncopy): d_i = dcat's slot i; the B * Cm / 64 blocks after them: dpool[b][64 channels] = sum over the
// image's rows, four row lanes per channel combined in lane order
template <typename T>
__global__ __launch_bounds__(256) void easpp_concat_bwd_kernel(const T* __restrict__ dcat, T* __restrict__ d0,
                                                         T* __restrict__ d1, T* __restrict__ d2, T* __restrict__ d3,
                                                         float* __restrict__ dpool, long M, int N, int Cm, int ncopy) {
  constexpr int V = VecT<T>::N;
  if ((int)blockIdx.x < ncopy) {
    const int vpr = 4 * Cm / V, vps = Cm / V;
    const long nvec = M * vpr;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (long)ncopy * 256) {
      const long row = i / vpr;
      const int cv = (int)(i % vpr), slot = cv / vps, c = (cv % vps) * V;
      T* dst = slot == 0 ? d0 : slot == 1 ? d1 : slot == 2 ? d2 : d3;
      *reinterpret_cast<Raw<T>*>(dst + row * Cm + c) = load_raw<T>(dcat + row * 5 * Cm + (long)slot * Cm + c);
    }
    return;
  }
  __shared__ float red[4][64];
  const int blk = blockIdx.x - ncopy, b = blk / (Cm / 64), c = (blk % (Cm / 64)) * 64 + (threadIdx.x & 63);
  const int q = threadIdx.x >> 6;
  float t = 0.f;
  for (int n = q; n < N; n += 4) t += to_f32(dcat[((long)b * N + n) * 5 * Cm + 4 * Cm + c]);
  red[q][threadIdx.x & 63] = t;
  __syncthreads();
  if (q == 0) {
    const int l = threadIdx.x;
    dpool[(long)b * Cm + c] = ((red[0][l] + red[1][l]) + red[2][l]) + red[3][l];
  }
}

// dx[b][n][c] = (1/N) sum_s part[s*ss + b*C + c]; blockIdx = (64 vector columns, image, row group)
template <typename T>
__global__ __launch_bounds__(256) void easpp_pool_bwd_kernel(const float* __restrict__ part, int nsl, long ss,
                                                       T* __restrict__ dx, int N, int C) {
  constexpr int V = VecT<T>::N;
  const int cv = blockIdx.x * 64 + (threadIdx.x & 63), b = blockIdx.y;
  if (cv * V >= C) return;
  float v[V];
#pragma unroll
  for (int j = 0; j < V; ++j) {
    float t = 0.f;
    for (int s = 0; s < nsl; ++s) t += part[s * ss + (long)b * C + cv * V + j];
    v[j] = t / N;
  }
  for (int n = blockIdx.z * 4 + (threadIdx.x >> 6); n < N; n += gridDim.z * 4)
    store_vec<T>(dx + ((long)b * N + n) * C + cv * V, v);
}

__global__ __launch_bounds__(256) void easpp_dropout_mask_kernel(float* __restrict__ m, long n, float p,
                                                           unsigned long long seed, unsigned long long* state) {
  const unsigned long long st = state[0];
  const float keep = 1.f / (1.f - p);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256)
    m[i] = u01(seed, st, (unsigned long long)i) >= p ? keep : 0.f;
  // every block read the step before it took its ticket: the last one to arrive may advance it
  if (last_arrival(reinterpret_cast<unsigned*>(state + 1), gridDim.x) && threadIdx.x == 0) state[0] = st + 1;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the argument checks the three convolution entry points share; a / o: the activation-side pointers
int check_conv(const char* what, const void* const* a, const void* const* wt, const void* const* o, int B, int h, int w,
               int C, const int* rate, long lda, long ldo, int dtype, bool o_fp32) {
  CMX_REQUIRE(dtype >= 0 && dtype <= 2, CMX_ERR_DTYPE, "%s: unsupported dtype %d", what, dtype);
  CMX_REQUIRE(C == CW, CMX_ERR_SHAPE, "%s: C=%d (the branch width is %d)", what, C, CW);
  CMX_REQUIRE(B > 0 && h > 0 && w > 0 && (long)B * h * w < (1L << 31) - 64, CMX_ERR_SHAPE, "%s: B=%d h=%d w=%d", what,
              B, h, w);
  const int V = dtype == 0 ? 4 : 8;
  for (int g = 0; g < 3; ++g) {
    CMX_REQUIRE(a[g] && wt[g] && o[g], CMX_ERR_ARG, "%s: null operand of branch %d", what, g);
    CMX_REQUIRE(aligned16(a[g]) && aligned16(wt[g]) && aligned16(o[g]), CMX_ERR_ARG,
                "%s: branch %d has an operand off a 16-byte boundary", what, g);
    CMX_REQUIRE(rate[g] >= 1, CMX_ERR_ARG, "%s: rate %d of branch %d", what, rate[g], g);
  }
  CMX_REQUIRE(lda >= CW && lda % V == 0 && (o_fp32 || (ldo >= CW && ldo % V == 0)), CMX_ERR_ARG,
              "%s: row strides %ld / %ld (>= %d, multiples of %d)", what, lda, ldo, CW, V);
  return CMX_OK;
}

template <bool DGRAD>
int launch_conv(const char* what, const void* const* a, const void* const* wt, void* const* o, int B, int h, int w,
                int C, const int* rate, long lda, long ldo, int dtype, hipStream_t s) {
  const int st = check_conv(what, a, wt, (const void* const*)o, B, h, w, C, rate, lda, ldo, dtype, false);
  if (st != CMX_OK) return st;
  Group3 P;
  for (int g = 0; g < 3; ++g) { P.a[g] = a[g]; P.w[g] = wt[g]; P.o[g] = o[g]; P.rate[g] = rate[g]; }
  const dim3 grid(cdiv((long)B * h * w, 32), 3);
  CMX_DISPATCH(dtype, T, { hipLaunchKernelGGL((easpp_conv_kernel<T, DGRAD>), grid, dim3(64), 0, s, P, B, h, w, lda, ldo); });
  return cmx_check_launch(what);
}

int wg_nchunk(int B, int h, int w) { return (int)(((long)B * h * w + WG_ROWS - 1) / WG_ROWS); }

unsigned ew_blocks(long nvec) {
  const long nb = (nvec + 255) / 256;
  return (unsigned)(nb < 1 ? 1 : nb < 2048 ? nb : 2048);
}

}  // namespace

extern "C" {

int cmx_easpp_conv_fwd(const void* x0, const void* x1, const void* x2, const void* w0, const void* w1, const void* w2,
                       void* y0, void* y1, void* y2, int B, int h, int w, int C, int r0, int r1, int r2, int64_t ldx,
                       int64_t ldy, int dtype, hipStream_t s) {
  const void* a[3] = {x0, x1, x2};
  const void* wt[3] = {w0, w1, w2};
  void* o[3] = {y0, y1, y2};
  const int rate[3] = {r0, r1, r2};
  return launch_conv<false>("easpp_conv_fwd", a, wt, o, B, h, w, C, rate, (long)ldx, (long)ldy, dtype, s);
}

int cmx_easpp_conv_dgrad(const void* dy0, const void* dy1, const void* dy2, const void* w0, const void* w1,
                         const void* w2, void* dx0, void* dx1, void* dx2, int B, int h, int w, int C, int r0, int r1,
                         int r2, int64_t lddy, int64_t lddx, int dtype, hipStream_t s) {
  const void* a[3] = {dy0, dy1, dy2};
  const void* wt[3] = {w0, w1, w2};
  void* o[3] = {dx0, dx1, dx2};
  const int rate[3] = {r0, r1, r2};
  return launch_conv<true>("easpp_conv_dgrad", a, wt, o, B, h, w, C, rate, (long)lddy, (long)lddx, dtype, s);
}

size_t cmx_easpp_conv_wgrad_workspace(int B, int h, int w) {
  if (B <= 0 || h <= 0 || w <= 0) return 0;
  const int nc = wg_nchunk(B, h, w);
  return nc > 1 ? (size_t)3 * nc * WSZ * sizeof(float) : 0;
}

int cmx_easpp_conv_wgrad(const void* dy0, const void* dy1, const void* dy2, const void* x0, const void* x1,
                         const void* x2, float* dw0, float* dw1, float* dw2, float* workspace, int B, int h, int w, int C,
                         int r0, int r1, int r2, int64_t lddy, int64_t ldx, int dtype, hipStream_t s) {
  const void* a[3] = {dy0, dy1, dy2};
  const void* xs[3] = {x0, x1, x2};
  const void* o[3] = {dw0, dw1, dw2};
  const int rate[3] = {r0, r1, r2};
  int st = check_conv("easpp_conv_wgrad", a, xs, o, B, h, w, C, rate, (long)lddy, 0, dtype, true);
  if (st != CMX_OK) return st;
  const int V = dtype == 0 ? 4 : 8;
  CMX_REQUIRE(ldx >= CW && ldx % V == 0, CMX_ERR_ARG, "easpp_conv_wgrad: row stride %ld", (long)ldx);
  const int nc = wg_nchunk(B, h, w);
  CMX_REQUIRE(nc == 1 || (workspace && aligned16(workspace)), CMX_ERR_ARG, "easpp_conv_wgrad: null workspace");
  Group3 P;
  for (int g = 0; g < 3; ++g) { P.a[g] = a[g]; P.w[g] = xs[g]; P.o[g] = (void*)o[g]; P.rate[g] = rate[g]; }
  CMX_DISPATCH(dtype, T, {
    hipLaunchKernelGGL(easpp_wgrad_kernel<T>, dim3(nc, TAPS, 3), dim3(64), 0, s, P, workspace, nc, B, h, w, (long)lddy,
                       (long)ldx);
  });
  st = cmx_check_launch("easpp_conv_wgrad");
  if (st != CMX_OK || nc == 1) return st;
  hipLaunchKernelGGL(easpp_fold3_kernel, dim3(WSZ / (256 * 4), 3), dim3(256), 0, s, workspace, dw0, dw1, dw2, nc);
  return cmx_check_launch("easpp_conv_wgrad fold");
}

int cmx_easpp_concat_fwd(const void* y0, const void* y1, const void* y2, const void* y3, const float* pool, void* cat,
                         int B, int N, int Cm, int dtype, hipStream_t s) {
  CMX_REQUIRE(y0 && y1 && y2 && y3 && pool && cat, CMX_ERR_ARG, "easpp_concat_fwd: null operand");
  CMX_REQUIRE(B > 0 && N > 0 && Cm > 0 && Cm % 64 == 0, CMX_ERR_SHAPE, "easpp_concat_fwd: B=%d N=%d Cm=%d", B, N, Cm);
  CMX_REQUIRE(aligned16(y0) && aligned16(y1) && aligned16(y2) && aligned16(y3) && aligned16(cat), CMX_ERR_ARG,
              "easpp_concat_fwd: an operand off a 16-byte boundary");
  const long M = (long)B * N;
  CMX_DISPATCH(dtype, T, {
    hipLaunchKernelGGL(easpp_concat_fwd_kernel<T>, dim3(ew_blocks(M * 5 * Cm / VecT<T>::N)), dim3(256), 0, s, (const T*)y0,
                       (const T*)y1, (const T*)y2, (const T*)y3, pool, (T*)cat, M, N, Cm);
  });
  return cmx_check_launch("easpp_concat_fwd");
}

int cmx_easpp_concat_bwd(const void* dcat, void* d0, void* d1, void* d2, void* d3, float* dpool, int B, int N, int Cm,
                         int dtype, hipStream_t s) {
  CMX_REQUIRE(dcat && d0 && d1 && d2 && d3 && dpool, CMX_ERR_ARG, "easpp_concat_bwd: null operand");
  CMX_REQUIRE(B > 0 && N > 0 && Cm > 0 && Cm % 64 == 0, CMX_ERR_SHAPE, "easpp_concat_bwd: B=%d N=%d Cm=%d", B, N, Cm);
  CMX_REQUIRE(aligned16(dcat) && aligned16(d0) && aligned16(d1) && aligned16(d2) && aligned16(d3), CMX_ERR_ARG,
              "easpp_concat_bwd: an operand off a 16-byte boundary");
  const long M = (long)B * N;
  CMX_DISPATCH(dtype, T, {
    const int ncopy = (int)ew_blocks(M * 4 * Cm / VecT<T>::N);
    hipLaunchKernelGGL(easpp_concat_bwd_kernel<T>, dim3(ncopy + B * (Cm / 64)), dim3(256), 0, s, (const T*)dcat, (T*)d0,
                       (T*)d1, (T*)d2, (T*)d3, dpool, M, N, Cm, ncopy);
  });
  return cmx_check_launch("easpp_concat_bwd");
}

int cmx_easpp_pool_bwd(const float* dpooled_part, int nslice, int64_t slice_stride, void* dx, int B, int N, int C,
                       int dtype, hipStream_t s) {
  CMX_REQUIRE(dpooled_part && dx, CMX_ERR_ARG, "easpp_pool_bwd: null operand");
  CMX_REQUIRE(B > 0 && N > 0 && C > 0 && C % 8 == 0 && nslice > 0 && nslice <= 16, CMX_ERR_SHAPE,
              "easpp_pool_bwd: B=%d N=%d C=%d nslice=%d", B, N, C, nslice);
  CMX_REQUIRE(aligned16(dx), CMX_ERR_ARG, "easpp_pool_bwd: dx off a 16-byte boundary");
  const int rowgroups = (N + 3) / 4 < 16 ? (N + 3) / 4 : 16;
  CMX_DISPATCH(dtype, T, {
    hipLaunchKernelGGL(easpp_pool_bwd_kernel<T>, dim3(cdiv(C / VecT<T>::N, 64), B, rowgroups), dim3(256), 0, s, dpooled_part,
                       nslice, (long)slice_stride, (T*)dx, N, C);
  });
  return cmx_check_launch("easpp_pool_bwd");
}

int cmx_easpp_dropout_mask(float* dscale, int64_t n, float p, uint64_t seed, uint64_t* state, hipStream_t s) {
  CMX_REQUIRE(dscale && state, CMX_ERR_ARG, "easpp_dropout_mask: null operand");
  CMX_REQUIRE(n > 0 && p >= 0.f && p < 1.f, CMX_ERR_ARG, "easpp_dropout_mask: n=%ld p=%f", (long)n, p);
  hipLaunchKernelGGL(easpp_dropout_mask_kernel, dim3(ew_blocks(n)), dim3(256), 0, s, dscale, (long)n, p,
                     (unsigned long long)seed, (unsigned long long*)state);
  return cmx_check_launch("easpp_dropout_mask");
}

}  // extern "C"
