// The DeepLabV3+ decoder's F.interpolate(c4, c1.size()[2:], mode='bilinear', align_corners=True) + torch.cat([c4, c1], 1)
// (deeplabv3plus.py:32-33) as one launch each way (include/cmx_deeplab.h).  Every other bilinear kernel of the library
// follows the align_corners=False rule; the BatchNorm kernels take no row stride, so the concat is a buffer.
//
//   upcat_ac_fwd_kernel<T>: cat row = [up_ac(lo) | skip], one 16-B vector per thread (HBM-bound: it writes the
//     (B H W, C + Cs) buffer once and reads lo, which sits in L2, four times).
//   upcat_ac_bwd_kernel<T>: blocks [0, ncopy): dskip = dcat's columns [C, C + Cs); the blocks after them: dlo as a
//     gather.  A low-res pixel (r, c) collects every output pixel whose taps touch it; the candidate rows and columns
//     come from the inverse of src = scale * Y widened by one, and each candidate's indices and weights are computed
//     by the forward's own rule, so the adjoint matches the forward whatever the rounding of scale * Y.  The
//     candidate rows are dealt to the block's four waves; the four partial sums are added in wave order.
// No atomics: bit-identical from run to run.
#include "cmx_common.h"
#include "../../include/cmx_deeplab.h"  // compiler-checks the definitions below against the ABI header

namespace {

// torch's align_corners=True source of output index `dst`: i0 = min(floor(scale dst), in - 1), i1 = min(i0 + 1, in - 1)
__device__ __forceinline__ void ac_src(int dst, float scale, int in, int& i0, int& i1, float& l0, float& l1) {
  const float s = scale * (float)dst;
  i0 = (int)s;
  if (i0 > in - 1) i0 = in - 1;
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = s - (float)i0;
  l0 = 1.f - l1;
}

// the weight output index `dst` gives input index `i`
__device__ __forceinline__ float ac_weight(int dst, float scale, int in, int i) {
  int i0, i1;
  float l0, l1;
  ac_src(dst, scale, in, i0, i1, l0, l1);
  return (i0 == i ? l0 : 0.f) + (i1 == i ? l1 : 0.f);
}

// the output indices [lo, hi] outside of which ac_weight(., scale, in, i) is zero (a superset)
__device__ __forceinline__ void ac_range(int i, float scale, int out, int& lo, int& hi) {
  lo = 0;
  hi = out - 1;
  if (scale > 0.f) {
    const float a = floorf((float)(i - 1) / scale) - 1.f, b = ceilf((float)(i + 1) / scale) + 1.f;
    if (a > 0.f) lo = (int)fminf(a, (float)(out - 1));
    if (b < (float)(out - 1)) hi = (int)b;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void upcat_ac_fwd_kernel(const T* __restrict__ lo, const T* __restrict__ skip,
                                                     T* __restrict__ cat, long M, int h, int w, int H, int W, int C,
                                                     int Cs, float sy, float sx) {
  constexpr int V = VecT<T>::N;
  const int vpr = (C + Cs) / V, vlo = C / V;
  const long nvec = M * vpr;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (long)gridDim.x * 256) {
    const long row = i / vpr;
    const int cv = (int)(i % vpr);
    T* dst = cat + row * (C + Cs) + (long)cv * V;
    if (cv >= vlo) {
      *reinterpret_cast<typename VecT<T>::raw*>(dst) = load_raw<T>(skip + row * Cs + (long)(cv - vlo) * V);
      continue;
    }
    const int X = (int)(row % W), Y = (int)((row / W) % H);
    const long b = row / ((long)W * H);
    int y0, y1, x0, x1;
    float ly0, ly1, lx0, lx1;
    ac_src(Y, sy, h, y0, y1, ly0, ly1);
    ac_src(X, sx, w, x0, x1, lx0, lx1);
    const T* base = lo + b * h * w * C + (long)cv * V;
    float v00[V], v01[V], v10[V], v11[V], o[V];
    load_vec<T>(base + ((long)y0 * w + x0) * C, v00);
    load_vec<T>(base + ((long)y0 * w + x1) * C, v01);
    load_vec<T>(base + ((long)y1 * w + x0) * C, v10);
    load_vec<T>(base + ((long)y1 * w + x1) * C, v11);
#pragma unroll
    for (int j = 0; j < V; ++j) o[j] = ly0 * (lx0 * v00[j] + lx1 * v01[j]) + ly1 * (lx0 * v10[j] + lx1 * v11[j]);
    store_vec<T>(dst, o);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void upcat_ac_bwd_kernel(const T* __restrict__ dcat, T* __restrict__ dlo,
                                                     T* __restrict__ dskip, long M, int B, int h, int w, int H, int W,
                                                     int C, int Cs, float sy, float sx, int ncopy) {
  constexpr int V = VecT<T>::N;
  const int Ct = C + Cs;
  if ((int)blockIdx.x < ncopy) {
    const int vps = Cs / V;
    const long nvec = M * vps;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (long)ncopy * 256) {
      const long row = i / vps;
      const int c = (int)(i % vps) * V;
      *reinterpret_cast<typename VecT<T>::raw*>(dskip + row * Cs + c) = load_raw<T>(dcat + row * Ct + C + c);
    }
    return;
  }
  __shared__ float red[3][64][V];
  const int vlo = C / V, q = threadIdx.x >> 6, l = threadIdx.x & 63;
  const long item = (long)(blockIdx.x - ncopy) * 64 + l, nitem = (long)B * h * w * vlo;
  const bool live = item < nitem;
  const long pixel = live ? item / vlo : 0;
  const int cv = live ? (int)(item % vlo) : 0;
  const int c = (int)(pixel % w), r = (int)((pixel / w) % h);
  const long b = pixel / ((long)w * h);
  float acc[V];
#pragma unroll
  for (int j = 0; j < V; ++j) acc[j] = 0.f;
  if (live) {
    int Y0, Y1, X0, X1;
    ac_range(r, sy, H, Y0, Y1);
    ac_range(c, sx, W, X0, X1);
    const T* base = dcat + b * H * W * Ct + (long)cv * V;
    for (int Y = Y0 + q; Y <= Y1; Y += 4) {
      const float wy = ac_weight(Y, sy, h, r);
      if (wy == 0.f) continue;
      for (int X = X0; X <= X1; ++X) {
        const float wgt = wy * ac_weight(X, sx, w, c);
        if (wgt == 0.f) continue;
        float v[V];
        load_vec<T>(base + ((long)Y * W + X) * Ct, v);
#pragma unroll
        for (int j = 0; j < V; ++j) acc[j] += wgt * v[j];
      }
    }
  }
  if (q > 0) {
#pragma unroll
    for (int j = 0; j < V; ++j) red[q - 1][l][j] = acc[j];
  }
  __syncthreads();
  if (q == 0 && live) {
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] = ((acc[j] + red[0][l][j]) + red[1][l][j]) + red[2][l][j];
    store_vec<T>(dlo + pixel * C + (long)cv * V, acc);
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

unsigned ew_blocks(long nvec) {
  const long nb = (nvec + 255) / 256;
  return (unsigned)(nb < 1 ? 1 : nb < 4096 ? nb : 4096);
}

int check(const char* what, const void* a, const void* b, const void* c, int B, int h, int w, int H, int W, int C, int Cs,
          int dtype) {
  CMX_REQUIRE(dtype >= 0 && dtype <= 2, CMX_ERR_DTYPE, "%s: unsupported dtype %d", what, dtype);
  CMX_REQUIRE(a && b && c, CMX_ERR_ARG, "%s: null operand", what);
  CMX_REQUIRE(B > 0 && h > 0 && w > 0 && h <= H && w <= W && C > 0 && C % 64 == 0 && Cs > 0 && Cs % 8 == 0 &&
              (long)B * H * W < (1L << 31) && (long)B * H * W * (C + Cs) < (1L << 40), CMX_ERR_SHAPE,
              "%s: B=%d (h, w)=(%d, %d) (H, W)=(%d, %d) C=%d Cs=%d (h <= H, w <= W, C %% 64 == 0, Cs %% 8 == 0)", what, B,
              h, w, H, W, C, Cs);
  CMX_REQUIRE(aligned16(a) && aligned16(b) && aligned16(c), CMX_ERR_ARG, "%s: an operand off a 16-byte boundary", what);
  return CMX_OK;
}

float ac_scale(int in, int out) { return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f; }

}  // namespace

extern "C" {

int cmx_upcat_ac_fwd(const void* lo, const void* skip, void* cat, int B, int h, int w, int H, int W, int C, int Cs,
                     int dtype, hipStream_t s) {
  const int st = check("upcat_ac_fwd", lo, skip, cat, B, h, w, H, W, C, Cs, dtype);
  if (st != CMX_OK) return st;
  const long M = (long)B * H * W;
  CMX_DISPATCH(dtype, T, {
    hipLaunchKernelGGL(upcat_ac_fwd_kernel<T>, dim3(ew_blocks(M * (C + Cs) / VecT<T>::N)), dim3(256), 0, s, (const T*)lo,
                       (const T*)skip, (T*)cat, M, h, w, H, W, C, Cs, ac_scale(h, H), ac_scale(w, W));
  });
  return cmx_check_launch("upcat_ac_fwd");
}

int cmx_upcat_ac_bwd(const void* dcat, void* dlo, void* dskip, int B, int h, int w, int H, int W, int C, int Cs, int dtype,
                     hipStream_t s) {
  const int st = check("upcat_ac_bwd", dcat, dlo, dskip, B, h, w, H, W, C, Cs, dtype);
  if (st != CMX_OK) return st;
  const long M = (long)B * H * W;
  CMX_DISPATCH(dtype, T, {
    const int ncopy = (int)ew_blocks(M * Cs / VecT<T>::N);
    const long nitem = (long)B * h * w * (C / VecT<T>::N);
    hipLaunchKernelGGL(upcat_ac_bwd_kernel<T>, dim3(ncopy + cdiv(nitem, 64)), dim3(256), 0, s, (const T*)dcat, (T*)dlo,
                       (T*)dskip, M, B, h, w, H, W, C, Cs, ac_scale(h, H), ac_scale(w, W), ncopy);
  });
  return cmx_check_launch("upcat_ac_bwd");
}

}  // extern "C"
