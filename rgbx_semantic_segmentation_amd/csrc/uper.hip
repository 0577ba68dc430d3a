// The UPerNet decode head's own launches (include/cmx_uper.h; models/decoders/UPernet.py), all HBM-bound: one 16-B
// vector per lane, channels innermost, no atomics, every sum in a fixed order.
//
//   ppm_pool_fwd_kernel<T>:   AdaptiveAvgPool2d at up to four scales, one thread per (bin, 16-B channel vector): the
//     bin's pixels are summed in row-major order in fp32 and divided by their count.  The stage-4 map is small (600
//     rows at B2 480 x 640) and sits in L2.
//   ppm_pool_bwd_kernel<T>:   one thread per (pixel, vector) gathers the bins that hold the pixel (at most a few per
//     scale; torch's bins overlap) on top of the optional `add` rows.
//   upcat_fwd_kernel<T>:      cat row = [skip | up(src_0) | ... ], align_corners=False, weights by cmx_bilin_src (the
//     rule of cmx_bilinear_fwd_nhwc).
//   upcat_bwd_kernel<T>:      blocks [0, ncopy): dskip = dcat's columns [0, Cs); the blocks after them: dsrc_i as a
//     gather.  A low-res pixel (r, c) collects every output pixel whose taps touch it: the candidate rows and columns
//     come from the inverse of the source rule widened by one, each candidate's weight from cmx_bilin_src itself, so
//     the adjoint matches the forward whatever the rounding of src.  The candidate rows are dealt to the block's four
//     waves; the four partial sums are added in wave order.
//   up_add_fwd_kernel<T>:     out = hi + up(lo).
//   flip_weight_kernel:       Wf[ci][T - 1 - t][co] = W[co][t][ci] on 16-bit words, 64 x 64 tiles through LDS.
// The per-source geometry travels by value and is only ever indexed with constants (unrolled selects), so nothing
// lives in scratch.
#include "cmx_common.h"
#include "../../include/cmx_uper.h"  // compiler-checks the definitions below against the ABI header

namespace {

struct PpmScales {
  int n;          // scales in use
  int s[4];       // bins per side
  int row0[5];    // first pooled row of scale k for B = 1 (sum of s_j^2, j < k); row0[n] = rows per image
};

struct UpSrcs {
  const void* p[4];
  int h[4], w[4];
  float sy[4], sx[4];   // (float)h / H, (float)w / W, as cmx_bilinear_fwd_nhwc forms them
  long item0[5];        // bwd: first gather item of source q
};

__device__ __forceinline__ int bin_lo(int i, int len, int s) { return (i * len) / s; }
__device__ __forceinline__ int bin_hi(int i, int len, int s) { return ((i + 1) * len + s - 1) / s; }

template <typename T>
__global__ __launch_bounds__(256) void ppm_pool_fwd_kernel(const T* __restrict__ x, T* __restrict__ pooled, int B, int h,
                                                           int w, int C, PpmScales sc) {
  constexpr int V = VecT<T>::N;
  const int vpr = C / V;
  const long nitem = (long)B * sc.row0[sc.n] * vpr;
  for (long it = (long)blockIdx.x * 256 + threadIdx.x; it < nitem; it += (long)gridDim.x * 256) {
    const int cv = (int)(it % vpr);
    const long row = it / vpr;
    int s = sc.s[0];
    long first = 0;
#pragma unroll
    for (int k = 1; k < 4; ++k)
      if (k < sc.n && row >= (long)B * sc.row0[k]) {
        s = sc.s[k];
        first = (long)B * sc.row0[k];
      }
    const int rr = (int)(row - first);
    const int j = rr % s, i = (rr / s) % s, b = rr / (s * s);
    const int ys = bin_lo(i, h, s), ye = bin_hi(i, h, s), xs = bin_lo(j, w, s), xe = bin_hi(j, w, s);
    const T* base = x + (long)b * h * w * C + (long)cv * V;
    float acc[V], v[V];
#pragma unroll
    for (int e = 0; e < V; ++e) acc[e] = 0.f;
    for (int yy = ys; yy < ye; ++yy) {
#pragma unroll 4
      for (int xx = xs; xx < xe; ++xx) {
        load_vec<T>(base + ((long)yy * w + xx) * C, v);
#pragma unroll
        for (int e = 0; e < V; ++e) acc[e] += v[e];
      }
    }
    const float cnt = (float)((ye - ys) * (xe - xs));
#pragma unroll
    for (int e = 0; e < V; ++e) acc[e] = acc[e] / cnt;
    store_vec<T>(pooled + row * C + (long)cv * V, acc);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void ppm_pool_bwd_kernel(const T* __restrict__ dpooled, const T* __restrict__ add,
                                                           long ldadd, T* __restrict__ dx, int B, int h, int w, int C,
                                                           PpmScales sc) {
  constexpr int V = VecT<T>::N;
  const int vpr = C / V;
  const long nitem = (long)B * h * w * vpr;
  for (long it = (long)blockIdx.x * 256 + threadIdx.x; it < nitem; it += (long)gridDim.x * 256) {
    const int cv = (int)(it % vpr);
    const long pix = it / vpr;
    const int xx = (int)(pix % w), yy = (int)((pix / w) % h), b = (int)(pix / ((long)w * h));
    float acc[V], v[V];
    if (add) {
      load_vec<T>(add + pix * ldadd + (long)cv * V, acc);
    } else {
#pragma unroll
      for (int e = 0; e < V; ++e) acc[e] = 0.f;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k >= sc.n) break;
      const int s = sc.s[k];
      const T* blk = dpooled + ((long)B * sc.row0[k] + (long)b * s * s) * C + (long)cv * V;
      for (int i = 0; i < s; ++i) {
        const int ys = bin_lo(i, h, s), ye = bin_hi(i, h, s);
        if (yy < ys || yy >= ye) continue;
        for (int j = 0; j < s; ++j) {
          const int xs = bin_lo(j, w, s), xe = bin_hi(j, w, s);
          if (xx < xs || xx >= xe) continue;
          const float cnt = (float)((ye - ys) * (xe - xs));
          load_vec<T>(blk + (long)(i * s + j) * C, v);
#pragma unroll
          for (int e = 0; e < V; ++e) acc[e] += v[e] / cnt;
        }
      }
    }
    store_vec<T>(dx + pix * C + (long)cv * V, acc);
  }
}

// the bilinear value of one 16-B vector at output pixel (Y, X) of a (h, w) source image `base` (row pitch C)
template <typename T>
__device__ __forceinline__ void bilin_vec(const T* base, int Y, int X, int h, int w, int C, float sy, float sx, float* o) {
  constexpr int V = VecT<T>::N;
  int y0, y1, x0, x1;
  float ly0, ly1, lx0, lx1;
  cmx_bilin_src(Y, sy, h, y0, y1, ly0, ly1);
  cmx_bilin_src(X, sx, w, x0, x1, lx0, lx1);
  float a[V], b[V], c[V], d[V];
  load_vec<T>(base + ((long)y0 * w + x0) * C, a);
  load_vec<T>(base + ((long)y0 * w + x1) * C, b);
  load_vec<T>(base + ((long)y1 * w + x0) * C, c);
  load_vec<T>(base + ((long)y1 * w + x1) * C, d);
#pragma unroll
  for (int j = 0; j < V; ++j) o[j] = ly0 * (lx0 * a[j] + lx1 * b[j]) + ly1 * (lx0 * c[j] + lx1 * d[j]);
}

// the weight output index `dst` gives input index `i` under cmx_bilin_src
__device__ __forceinline__ float bl_weight(int dst, float scale, int in, int i) {
  int i0, i1;
  float l0, l1;
  cmx_bilin_src(dst, scale, in, i0, i1, l0, l1);
  return (i0 == i ? l0 : 0.f) + (i1 == i ? l1 : 0.f);
}

// the output indices [lo, hi] outside of which bl_weight(., scale, in, i) is zero (a superset): src = (Y + 0.5) scale
// - 0.5 lies in [i - 1, i + 1), widened by one on each side; the clamps of the rule only move weight onto i = 0 from
// outputs below that range's start, which the lower clamp at 0 keeps.  Holds for any scale > 0: the PPM's 6 x 6 source
// on a stage-4 map smaller than that is a DOWNsample (scale > 1)
__device__ __forceinline__ void bl_range(int i, float scale, int out, int& lo, int& hi) {
  const float a = floorf(((float)i - 0.5f) / scale - 0.5f) - 1.f, b = ceilf(((float)i + 1.5f) / scale - 0.5f) + 1.f;
  lo = a > 0.f ? (int)fminf(a, (float)(out - 1)) : 0;
  hi = b < (float)(out - 1) ? (int)b : out - 1;
}

template <typename T>
__global__ __launch_bounds__(256) void upcat_fwd_kernel(const T* __restrict__ skip, T* __restrict__ cat, long M, int H,
                                                        int W, int Cs, int C, int n, UpSrcs sr) {
  constexpr int V = VecT<T>::N;
  const int vs = Cs / V, vc = C / V, vpr = vs + n * vc;
  const long Ct = (long)Cs + (long)n * C;
  const long nvec = M * vpr;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (long)gridDim.x * 256) {
    const long row = i / vpr;
    const int cv = (int)(i % vpr);
    T* dst = cat + row * Ct + (long)cv * V;
    if (cv < vs) {
      *reinterpret_cast<typename VecT<T>::raw*>(dst) = load_raw<T>(skip + row * Cs + (long)cv * V);
      continue;
    }
    const int q = (cv - vs) / vc, cq = (cv - vs) % vc;
    const T* p = (const T*)sr.p[0];
    int h = sr.h[0], w = sr.w[0];
    float sy = sr.sy[0], sx = sr.sx[0];
#pragma unroll
    for (int k = 1; k < 4; ++k)
      if (q == k) {
        p = (const T*)sr.p[k];
        h = sr.h[k];
        w = sr.w[k];
        sy = sr.sy[k];
        sx = sr.sx[k];
      }
    const int X = (int)(row % W), Y = (int)((row / W) % H);
    const long b = row / ((long)W * H);
    float o[V];
    bilin_vec<T>(p + b * h * w * C + (long)cq * V, Y, X, h, w, C, sy, sx, o);
    store_vec<T>(dst, o);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void upcat_bwd_kernel(const T* __restrict__ dcat, T* __restrict__ dskip, long M, int B,
                                                        int H, int W, int Cs, int C, int n, int ncopy, UpSrcs sr) {
  constexpr int V = VecT<T>::N;
  const long Ct = (long)Cs + (long)n * C;
  if ((int)blockIdx.x < ncopy) {
    const int vps = Cs / V;
    const long nvec = M * vps;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (long)ncopy * 256) {
      const long row = i / vps;
      const int c = (int)(i % vps) * V;
      *reinterpret_cast<typename VecT<T>::raw*>(dskip + row * Cs + c) = load_raw<T>(dcat + row * Ct + c);
    }
    return;
  }
  __shared__ float red[3][64][V];
  const int vc = C / V, wv = threadIdx.x >> 6, l = threadIdx.x & 63;
  const long item = (long)(blockIdx.x - ncopy) * 64 + l;
  const bool live = item < sr.item0[n];
  int q = 0;
  T* out = (T*)sr.p[0];
  int h = sr.h[0], w = sr.w[0];
  float sy = sr.sy[0], sx = sr.sx[0];
  long first = 0;
#pragma unroll
  for (int k = 1; k < 4; ++k)
    if (k < n && item >= sr.item0[k]) {
      q = k;
      out = (T*)sr.p[k];
      h = sr.h[k];
      w = sr.w[k];
      sy = sr.sy[k];
      sx = sr.sx[k];
      first = sr.item0[k];
    }
  const long local = live ? item - first : 0;
  const long pixel = local / vc;
  const int cv = (int)(local % vc);
  const int c = (int)(pixel % w), r = (int)((pixel / w) % h);
  const long b = pixel / ((long)w * h);
  float acc[V];
#pragma unroll
  for (int j = 0; j < V; ++j) acc[j] = 0.f;
  if (live) {
    int Y0, Y1, X0, X1;
    bl_range(r, sy, H, Y0, Y1);
    bl_range(c, sx, W, X0, X1);
    const T* base = dcat + b * H * W * Ct + Cs + (long)q * C + (long)cv * V;
    for (int Y = Y0 + wv; Y <= Y1; Y += 4) {
      const float wy = bl_weight(Y, sy, h, r);
      if (wy == 0.f) continue;
      for (int X = X0; X <= X1; ++X) {
        const float wgt = wy * bl_weight(X, sx, w, c);
        if (wgt == 0.f) continue;
        float v[V];
        load_vec<T>(base + ((long)Y * W + X) * Ct, v);
#pragma unroll
        for (int j = 0; j < V; ++j) acc[j] += wgt * v[j];
      }
    }
  }
  if (wv > 0) {
#pragma unroll
    for (int j = 0; j < V; ++j) red[wv - 1][l][j] = acc[j];
  }
  __syncthreads();
  if (wv == 0 && live) {
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] = ((acc[j] + red[0][l][j]) + red[1][l][j]) + red[2][l][j];
    store_vec<T>(out + pixel * C + (long)cv * V, acc);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void up_add_fwd_kernel(const T* __restrict__ hi, const T* __restrict__ lo,
                                                         T* __restrict__ out, long M, int h, int w, int H, int W, int C,
                                                         float sy, float sx) {
  constexpr int V = VecT<T>::N;
  const int vpr = C / V;
  const long nvec = M * vpr;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (long)gridDim.x * 256) {
    const long row = i / vpr;
    const int cv = (int)(i % vpr);
    const int X = (int)(row % W), Y = (int)((row / W) % H);
    const long b = row / ((long)W * H);
    float o[V], a[V];
    load_vec<T>(hi + row * C + (long)cv * V, a);
    bilin_vec<T>(lo + b * h * w * C + (long)cv * V, Y, X, h, w, C, sy, sx, o);
#pragma unroll
    for (int j = 0; j < V; ++j) o[j] = a[j] + o[j];
    store_vec<T>(out + row * C + (long)cv * V, o);
  }
}

// one 64 (co) x 64 (ci) tile of tap blockIdx.z: 16-B loads along ci, 16-B stores along co.  LDS rows are 66 halfwords
// (33 dwords: an odd pitch, so the column reads of eight consecutive co spread over the banks)
constexpr int FT = 64, FP = FT + 2;

__global__ __launch_bounds__(256) void flip_weight_kernel(const uint16_t* __restrict__ Wt, uint16_t* __restrict__ Wf,
                                                          int N, int T, int C, long ldw) {
  __shared__ uint16_t tile[FT][FP];
  const int co0 = blockIdx.x * FT, ci0 = blockIdx.y * FT, t = blockIdx.z;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int v = threadIdx.x + k * 256;        // 512 vectors: 64 rows (co) of 8
    const int r = v >> 3, cvec = (v & 7) * 8;
    if (ci0 + cvec < C) {
      const uint4 u = *reinterpret_cast<const uint4*>(Wt + (long)(co0 + r) * ldw + (long)t * C + ci0 + cvec);
      uint32_t* d = reinterpret_cast<uint32_t*>(&tile[r][cvec]);
      d[0] = u.x; d[1] = u.y; d[2] = u.z; d[3] = u.w;
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int v = threadIdx.x + k * 256;        // 512 vectors: 64 rows (ci) of 8 (co)
    const int r = v >> 3, cvec = (v & 7) * 8;
    if (ci0 + r < C) {
      uint32_t o[4];
#pragma unroll
      for (int e = 0; e < 4; ++e)
        o[e] = (uint32_t)tile[cvec + 2 * e][r] | ((uint32_t)tile[cvec + 2 * e + 1][r] << 16);
      *reinterpret_cast<uint4*>(Wf + ((long)(ci0 + r) * T + (T - 1 - t)) * N + co0 + cvec) =
          make_uint4(o[0], o[1], o[2], o[3]);
    }
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

unsigned ew_blocks(long nitem) {
  const long nb = (nitem + 255) / 256;
  return (unsigned)(nb < 1 ? 1 : nb < 4096 ? nb : 4096);
}

int ppm_scales(const char* what, int s0, int s1, int s2, int s3, PpmScales& sc) {
  const int s[4] = {s0, s1, s2, s3};
  sc.n = 0;
  sc.row0[0] = 0;
  for (int k = 0; k < 4; ++k) {
    sc.s[k] = 1;
    sc.row0[k + 1] = sc.row0[k];
  }
  for (int k = 0; k < 4; ++k) {
    if (s[k] == 0 && k > 0) {
      for (int j = k; j < 4; ++j)
        CMX_REQUIRE(s[j] == 0, CMX_ERR_SHAPE, "%s: scale %d given after an absent one", what, j);
      break;
    }
    CMX_REQUIRE(s[k] >= 1 && s[k] <= 8, CMX_ERR_SHAPE, "%s: scale %d = %d (1..8)", what, k, s[k]);
    sc.s[k] = s[k];
    sc.n = k + 1;
  }
  for (int k = 0; k < 4; ++k) sc.row0[k + 1] = sc.row0[k] + (k < sc.n ? sc.s[k] * sc.s[k] : 0);
  return CMX_OK;
}

int ppm_check(const char* what, const void* a, const void* b, int B, int h, int w, int C, int dtype) {
  CMX_REQUIRE(dtype >= 0 && dtype <= 2, CMX_ERR_DTYPE, "%s: unsupported dtype %d", what, dtype);
  CMX_REQUIRE(a && b, CMX_ERR_ARG, "%s: null operand", what);
  CMX_REQUIRE(B > 0 && h > 0 && w > 0 && C > 0 && C % 8 == 0 && (long)B * h * w < (1L << 31) &&
              (long)B * h * w * C < (1L << 40), CMX_ERR_SHAPE, "%s: B=%d (h, w)=(%d, %d) C=%d (C %% 8 == 0)", what, B, h,
              w, C);
  CMX_REQUIRE(aligned16(a) && aligned16(b), CMX_ERR_ARG, "%s: an operand off a 16-byte boundary", what);
  return CMX_OK;
}

// the shared checks of the upcat / up-add family; fills sr's geometry (item0 for the backward's gather)
int up_check(const char* what, int B, int H, int W, int Cs, int C, int n, const void* const* ps, const int* hs,
             const int* ws, int dtype, UpSrcs& sr) {
  CMX_REQUIRE(dtype >= 0 && dtype <= 2, CMX_ERR_DTYPE, "%s: unsupported dtype %d", what, dtype);
  CMX_REQUIRE(n >= 1 && n <= 4, CMX_ERR_SHAPE, "%s: %d sources (1..4)", what, n);
  CMX_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0 && Cs >= 0 && Cs % 8 == 0 &&
              (long)B * H * W < (1L << 31) && (long)B * H * W * ((long)Cs + (long)n * C) < (1L << 40), CMX_ERR_SHAPE,
              "%s: B=%d (H, W)=(%d, %d) Cs=%d C=%d (C %% 8 == 0, Cs %% 8 == 0)", what, B, H, W, Cs, C);
  sr.item0[0] = 0;
  for (int q = 0; q < 4; ++q) {
    const bool on = q < n;
    if (on) {
      CMX_REQUIRE(ps[q], CMX_ERR_ARG, "%s: source %d is null", what, q);
      CMX_REQUIRE(hs[q] >= 1 && ws[q] >= 1 && (long)B * hs[q] * ws[q] < (1L << 31), CMX_ERR_SHAPE,
                  "%s: source %d is (%d, %d)", what, q, hs[q], ws[q]);
      CMX_REQUIRE(aligned16(ps[q]), CMX_ERR_ARG, "%s: source %d off a 16-byte boundary", what, q);
    }
    sr.p[q] = on ? ps[q] : ps[0];
    sr.h[q] = on ? hs[q] : 1;
    sr.w[q] = on ? ws[q] : 1;
    sr.sy[q] = (float)sr.h[q] / (float)H;
    sr.sx[q] = (float)sr.w[q] / (float)W;
    sr.item0[q + 1] = sr.item0[q] + (on ? (long)B * hs[q] * ws[q] * (C / (dtype == 0 ? 4 : 8)) : 0);
  }
  return CMX_OK;
}

}  // namespace

extern "C" {

int cmx_ppm_pool_fwd(const void* x, void* pooled, int B, int h, int w, int C, int s0, int s1, int s2, int s3, int dtype,
                     hipStream_t s) {
  int st = ppm_check("ppm_pool_fwd", x, pooled, B, h, w, C, dtype);
  if (st != CMX_OK) return st;
  PpmScales sc;
  if ((st = ppm_scales("ppm_pool_fwd", s0, s1, s2, s3, sc)) != CMX_OK) return st;
  CMX_DISPATCH(dtype, T, {
    const long nitem = (long)B * sc.row0[sc.n] * (C / VecT<T>::N);
    hipLaunchKernelGGL(ppm_pool_fwd_kernel<T>, dim3(ew_blocks(nitem)), dim3(256), 0, s, (const T*)x, (T*)pooled, B, h, w,
                       C, sc);
  });
  return cmx_check_launch("ppm_pool_fwd");
}

int cmx_ppm_pool_bwd(const void* dpooled, const void* add, int64_t ldadd, void* dx, int B, int h, int w, int C, int s0,
                     int s1, int s2, int s3, int dtype, hipStream_t s) {
  int st = ppm_check("ppm_pool_bwd", dpooled, dx, B, h, w, C, dtype);
  if (st != CMX_OK) return st;
  PpmScales sc;
  if ((st = ppm_scales("ppm_pool_bwd", s0, s1, s2, s3, sc)) != CMX_OK) return st;
  CMX_REQUIRE(!add || (aligned16(add) && ldadd >= C && ldadd % 8 == 0), CMX_ERR_ARG,
              "ppm_pool_bwd: add off a 16-byte boundary, or its row stride %ld (>= C, a multiple of 8)", (long)ldadd);
  CMX_DISPATCH(dtype, T, {
    const long nitem = (long)B * h * w * (C / VecT<T>::N);
    hipLaunchKernelGGL(ppm_pool_bwd_kernel<T>, dim3(ew_blocks(nitem)), dim3(256), 0, s, (const T*)dpooled, (const T*)add,
                       (long)ldadd, (T*)dx, B, h, w, C, sc);
  });
  return cmx_check_launch("ppm_pool_bwd");
}

int cmx_upcat_multi_fwd(const void* skip, const void* src0, const void* src1, const void* src2, const void* src3,
                        void* cat, int B, int H, int W, int Cs, int C, int n, int h0, int w0, int h1, int w1, int h2,
                        int w2, int h3, int w3, int dtype, hipStream_t s) {
  const void* ps[4] = {src0, src1, src2, src3};
  const int hs[4] = {h0, h1, h2, h3}, ws[4] = {w0, w1, w2, w3};
  UpSrcs sr;
  const int st = up_check("upcat_multi_fwd", B, H, W, Cs, C, n, ps, hs, ws, dtype, sr);
  if (st != CMX_OK) return st;
  CMX_REQUIRE(cat && (Cs == 0 || skip), CMX_ERR_ARG, "upcat_multi_fwd: null operand");
  CMX_REQUIRE(aligned16(cat) && (Cs == 0 || aligned16(skip)), CMX_ERR_ARG,
              "upcat_multi_fwd: an operand off a 16-byte boundary");
  const long M = (long)B * H * W;
  CMX_DISPATCH(dtype, T, {
    hipLaunchKernelGGL(upcat_fwd_kernel<T>, dim3(ew_blocks(M * ((Cs + (long)n * C) / VecT<T>::N))), dim3(256), 0, s,
                       (const T*)skip, (T*)cat, M, H, W, Cs, C, n, sr);
  });
  return cmx_check_launch("upcat_multi_fwd");
}

int cmx_upcat_multi_bwd(const void* dcat, void* dskip, void* dsrc0, void* dsrc1, void* dsrc2, void* dsrc3, int B, int H,
                        int W, int Cs, int C, int n, int h0, int w0, int h1, int w1, int h2, int w2, int h3, int w3,
                        int dtype, hipStream_t s) {
  const void* ps[4] = {dsrc0, dsrc1, dsrc2, dsrc3};
  const int hs[4] = {h0, h1, h2, h3}, ws[4] = {w0, w1, w2, w3};
  UpSrcs sr;
  const int st = up_check("upcat_multi_bwd", B, H, W, Cs, C, n, ps, hs, ws, dtype, sr);
  if (st != CMX_OK) return st;
  CMX_REQUIRE(dcat, CMX_ERR_ARG, "upcat_multi_bwd: null operand");
  CMX_REQUIRE(aligned16(dcat) && aligned16(dskip), CMX_ERR_ARG, "upcat_multi_bwd: an operand off a 16-byte boundary");
  const long M = (long)B * H * W;
  CMX_DISPATCH(dtype, T, {
    const int ncopy = dskip && Cs > 0 ? (int)ew_blocks(M * (Cs / VecT<T>::N)) : 0;
    hipLaunchKernelGGL(upcat_bwd_kernel<T>, dim3(ncopy + cdiv(sr.item0[n], 64)), dim3(256), 0, s, (const T*)dcat,
                       (T*)dskip, M, B, H, W, Cs, C, n, ncopy, sr);
  });
  return cmx_check_launch("upcat_multi_bwd");
}

int cmx_up_add_fwd(const void* hi, const void* lo, void* out, int B, int h, int w, int H, int W, int C, int dtype,
                   hipStream_t s) {
  const void* ps[4] = {lo, nullptr, nullptr, nullptr};
  const int hs[4] = {h, 0, 0, 0}, ws[4] = {w, 0, 0, 0};
  UpSrcs sr;
  const int st = up_check("up_add_fwd", B, H, W, 0, C, 1, ps, hs, ws, dtype, sr);
  if (st != CMX_OK) return st;
  CMX_REQUIRE(hi && out, CMX_ERR_ARG, "up_add_fwd: null operand");
  CMX_REQUIRE(hi != out && lo != out, CMX_ERR_ARG, "up_add_fwd: out must be a buffer of its own");
  CMX_REQUIRE(aligned16(hi) && aligned16(out), CMX_ERR_ARG, "up_add_fwd: an operand off a 16-byte boundary");
  const long M = (long)B * H * W;
  CMX_DISPATCH(dtype, T, {
    hipLaunchKernelGGL(up_add_fwd_kernel<T>, dim3(ew_blocks(M * (C / VecT<T>::N))), dim3(256), 0, s, (const T*)hi,
                       (const T*)lo, (T*)out, M, h, w, H, W, C, sr.sy[0], sr.sx[0]);
  });
  return cmx_check_launch("up_add_fwd");
}

int cmx_conv_flip_weight(const void* W, void* Wf, int N, int KH, int KW, int C, int64_t ldw, int dtype, hipStream_t s) {
  CMX_REQUIRE(dtype == 1 || dtype == 2, CMX_ERR_DTYPE, "conv_flip_weight: 16-bit weights only (dtype %d)", dtype);
  CMX_REQUIRE(W && Wf, CMX_ERR_ARG, "conv_flip_weight: null operand");
  CMX_REQUIRE(N > 0 && N % 64 == 0 && C > 0 && C % 8 == 0 && KH > 0 && KW > 0 && (long)KH * KW <= 65535 &&
              (long)N * KH * KW * C < (1L << 40), CMX_ERR_SHAPE,
              "conv_flip_weight: N=%d (a multiple of 64) C=%d (a multiple of 8) taps (%d, %d)", N, C, KH, KW);
  CMX_REQUIRE(aligned16(W) && aligned16(Wf) && W != Wf && ldw >= (long)KH * KW * C && ldw % 8 == 0, CMX_ERR_ARG,
              "conv_flip_weight: an operand off a 16-byte boundary, or row stride %ld", (long)ldw);
  hipLaunchKernelGGL(flip_weight_kernel, dim3(N / FT, cdiv(C, FT), KH * KW), dim3(256), 0, s, (const uint16_t*)W,
                     (uint16_t*)Wf, N, KH * KW, C, (long)ldw);
  return cmx_check_launch("conv_flip_weight");
}

}  // extern "C"
