// Channel-attention (squeeze-excite) gate of the MLPDecoderpp decode head (MLPDecoderpp.py:55-61,
// 81-85) on the token-major fused map y (B, N, C), channels contiguous:
//
//     a   = sigmoid(W2 GELU(W1 avgpool_n(y) + b1) + b2)          (B, C) fp32
//     out = y * a[b, c] * dscale[b, c]                            dscale: the Dropout2d scale (NULLable)
//
//  pool        pooled[b][c] = (1/N) sum_n y[b][n][c]: block (z, tile, b) sums row chunk z of a
//              column tile to an fp32 partial; the last block of (tile, b) to arrive folds the
//              partials in chunk order (last_arrival, cmx_common.h).  No float atomics: the
//              result does not depend on the arrival order.
//  scale       out = y * (a * dscale): the per-(b, c) factor is formed once per thread, before
//              its row loop.
//  bwd_reduce  da[b][c] = dscale[b][c] * sum_n dout[b][n][c] y[b][n][c], left as one slice per row
//              chunk in the (dy_part, nslice, slice stride B*C, row stride C) form
//              cmx_small_linear_bwd sums itself: no fold launch.
//  bwd_apply   dy = dout * (a * dscale) + (1/N) sum_s dpool_part[s][b][c]: the gate path's
//              gradient arrives as the GEMV backward's dx slices and is summed here, once per
//              workgroup (as cmx_frm_pool_bwd does).
//  The gate MLP between them is cmx_small_linear_fwd / _bwd and cmx_act_fwd / _bwd on (B, C) fp32.
//
// All four are HBM streams of the largest decoder tensor (39 MB at B2 480 x 640 bf16): 16-B
// vectors along C, a row (or a 512-B / 256-B column tile of it) per group of consecutive lanes,
// four rows' loads in flight per thread before any is used.
#include "cmx_common.h"

namespace {

constexpr int SE_CHUNK = 64;                    // least rows per partial of the two reductions
constexpr int SE_NZ_MAX = 128;                  // most partials per (b, c): the fold and the GEMV
                                                // backward's prologue each read that many per value
constexpr int SE_RED_CW = 128;                  // channels per block of the two reductions
constexpr int SE_SL_MAX = 16;                   // dpool slices bwd_apply sums (cmx_small_linear_nslice)

// largest power of two dividing n, at most cap
inline int pow2_div(int n, int cap) {
  int p = 1;
  while (2 * p <= cap && n % (2 * p) == 0) p <<= 1;
  return p;
}
inline int se_nchunk(int N) {
  const long nz = ((long)N + SE_CHUNK - 1) / SE_CHUNK;
  return nz < 1 ? 1 : nz > SE_NZ_MAX ? SE_NZ_MAX : (int)nz;
}

// DOT = false: the sum of x over a row chunk (pool), folded over the chunks by the last block.
// DOT = true : the sum of x * d over a row chunk times dscale, written as slice z (bwd_reduce).
// Block (z, tile, b): cw channels = tw lanes x one 16-B vector, 256 / tw rows in flight.
template <typename T, bool DOT>
__global__ __launch_bounds__(256) void se_reduce_kernel(const T* __restrict__ x, const T* __restrict__ d,
                                                        const float* __restrict__ dscale, float* __restrict__ part,
                                                        float* __restrict__ pooled, unsigned* __restrict__ tickets,
                                                        int B, int N, int C, int cw, int chunk) {
  constexpr int V = VecT<T>::N;
  typedef typename VecT<T>::raw raw;
  __shared__ float red[256 * V];                // [row slot][cw]
  const int z = blockIdx.x, tile = blockIdx.y, b = blockIdx.z, nz = gridDim.x, ntile = gridDim.y;
  const int tw = cw / V, rpb = 256 / tw;
  const int lane = threadIdx.x % tw, slot = threadIdx.x / tw;
  const int n0 = z * chunk, n1 = min(N, n0 + chunk);
  const long base = (long)b * N * C + tile * cw + lane * V;
  float acc[V];
#pragma unroll
  for (int j = 0; j < V; ++j) acc[j] = 0.f;
  int n = n0 + slot;
  for (; n + 3 * rpb < n1; n += 4 * rpb) {      // four rows' loads in flight, added in row order
    raw rx[4], rd[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      rx[u] = load_raw<T>(x + base + (long)(n + u * rpb) * C);
      if constexpr (DOT) rd[u] = load_raw<T>(d + base + (long)(n + u * rpb) * C);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      float v[V], w[V];
      unpack_raw<T>(rx[u], v);
      if constexpr (DOT) {
        unpack_raw<T>(rd[u], w);
#pragma unroll
        for (int j = 0; j < V; ++j) acc[j] += v[j] * w[j];
      } else {
#pragma unroll
        for (int j = 0; j < V; ++j) acc[j] += v[j];
      }
    }
  }
  for (; n < n1; n += rpb) {
    float v[V], w[V];
    load_vec<T>(x + base + (long)n * C, v);
    if constexpr (DOT) {
      load_vec<T>(d + base + (long)n * C, w);
#pragma unroll
      for (int j = 0; j < V; ++j) acc[j] += v[j] * w[j];
    } else {
#pragma unroll
      for (int j = 0; j < V; ++j) acc[j] += v[j];
    }
  }
#pragma unroll
  for (int j = 0; j < V; ++j) red[slot * cw + lane * V + j] = acc[j];
  __syncthreads();
  const int c = threadIdx.x;                    // one thread per channel of the tile (cw <= 128)
  float t = 0.f;
  if (c < cw)
    for (int q = 0; q < rpb; ++q) t += red[q * cw + c];
  const long bc = (long)b * C + tile * cw + c;
  if constexpr (DOT) {
    if (c < cw) part[(long)z * B * C + bc] = dscale ? t * dscale[bc] : t;
  } else {
    float* pw = part + ((long)(b * ntile + tile) * nz) * cw;
    if (c < cw) st_agent(pw + (long)z * cw + c, t);
    if (!last_arrival(tickets + b * ntile + tile, nz)) return;
    // fold by the whole block: thread (fc, fp) sums the chunks fp, fp + P, ... (P = 256 / cw threads
    // per channel, sixteen partials in flight), the P sums combine through LDS in fp order -- a
    // fixed order whichever block folds.  (One thread per channel walking all nz partials was a
    // chain of nz / 8 dependent round trips: 10 us of a 23 us launch at B2 480 x 640.)
    const int P = 256 / cw, fc = threadIdx.x % cw, fp = threadIdx.x / cw;
    const float* pr = pw + fc;
    float s = 0.f;
    int zz = fp;
    for (; zz + 15 * P < nz; zz += 16 * P) {
      float t16[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) t16[u] = ld_agent(pr + (long)(zz + u * P) * cw);
#pragma unroll
      for (int u = 0; u < 16; ++u) s += t16[u];
    }
    for (; zz < nz; zz += P) s += ld_agent(pr + (long)zz * cw);
    red[fp * cw + fc] = s;                      // (red's earlier readers passed last_arrival's barriers)
    __syncthreads();
    if (c < cw) {
      float tot = 0.f;
      for (int q = 0; q < P; ++q) tot += red[q * cw + c];
      pooled[bc] = tot / (float)N;
    }
  }
}

// ADD = false: out = x * (a * dscale)                                    (scale)
// ADD = true : out = x * (a * dscale) + (1/N) sum_s part[s*ss + b*C + c] (bwd_apply)
// Block (row block, tile, b): tw lanes x one 16-B vector per row, 256 / tw rows in flight; the
// per-(b, c) terms are formed once per workgroup, before the row loop.
template <typename T, bool ADD>
__global__ __launch_bounds__(256) void se_stream_kernel(const T* __restrict__ x, const float* __restrict__ a,
                                                        const float* __restrict__ dscale,
                                                        const float* __restrict__ part, int nsl, long ss,
                                                        T* __restrict__ out, int B, int N, int C, int tw) {
  constexpr int V = VecT<T>::N;
  typedef typename VecT<T>::raw raw;
  const int tile = blockIdx.y, b = blockIdx.z;
  const int rpb = 256 / tw;
  const int lane = threadIdx.x % tw, slot = threadIdx.x / tw;
  const int c0 = (tile * tw + lane) * V;
  const long bc = (long)b * C + c0;
  float f[V], g[V];
#pragma unroll
  for (int j = 0; j < V; ++j) g[j] = 0.f;
  if constexpr (ADD) {
    // the block's tw * V (<= 512) pooled-gradient terms, each summed over the nsl (<= SE_SL_MAX)
    // slices in slice order, once per block: every slice's load issued before the sum
    // (unconditional, selected after), one channel per thread so a wave reads 256 B per slice
    __shared__ float sg[64 * V];
    for (int e = threadIdx.x; e < tw * V; e += 256) {
      const float* p = part + (long)b * C + tile * tw * V + e;
      float v[SE_SL_MAX];
#pragma unroll
      for (int q = 0; q < SE_SL_MAX; ++q) v[q] = p[(long)(q < nsl ? q : 0) * ss];
      float t = 0.f;
#pragma unroll
      for (int q = 0; q < SE_SL_MAX; ++q) t += q < nsl ? v[q] : 0.f;
      sg[e] = t / N;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < V; ++j) g[j] = sg[lane * V + j];
  }
#pragma unroll
  for (int k = 0; k < V / 4; ++k) {
    const float4 av = *reinterpret_cast<const float4*>(a + bc + 4 * k);
    float4 sv = make_float4(1.f, 1.f, 1.f, 1.f);
    if (dscale) sv = *reinterpret_cast<const float4*>(dscale + bc + 4 * k);
    f[4 * k] = av.x * sv.x; f[4 * k + 1] = av.y * sv.y; f[4 * k + 2] = av.z * sv.z; f[4 * k + 3] = av.w * sv.w;
  }
  const long base = (long)b * N * C + c0;
  const int st = gridDim.x * rpb;
  int n = blockIdx.x * rpb + slot;
  for (; (long)n + 3L * st < N; n += 4 * st) {  // four rows' loads in flight
    raw r[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) r[u] = load_raw<T>(x + base + (long)(n + u * st) * C);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      float v[V];
      unpack_raw<T>(r[u], v);
#pragma unroll
      for (int j = 0; j < V; ++j) v[j] = ADD ? v[j] * f[j] + g[j] : v[j] * f[j];
      store_vec<T>(out + base + (long)(n + u * st) * C, v);
    }
  }
  for (; n < N; n += st) {
    float v[V];
    load_vec<T>(x + base + (long)n * C, v);
#pragma unroll
    for (int j = 0; j < V; ++j) v[j] = ADD ? v[j] * f[j] + g[j] : v[j] * f[j];
    store_vec<T>(out + base + (long)n * C, v);
  }
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// shapes every entry point takes: C a multiple of 8 (a 16-B vector in each storage type), grid limits
inline bool se_shape_ok(int B, int N, int C) {
  return B > 0 && B <= 65535 && N > 0 && C > 0 && C % 8 == 0 && C <= 65536 && (long)N * 4 < (1L << 31);
}

template <bool ADD>
int se_stream(const void* x, const float* a, const float* dscale, const float* part, int nsl, long ss, void* out,
              int B, int N, int C, int dtype, hipStream_t s, const char* what) {
  const int V = dtype == 0 ? 4 : 8;
  const int tw = pow2_div(C / V, 64), rpb = 256 / tw, ntile = C / V / tw;
  long nb = ((long)N + 4L * rpb - 1) / (4L * rpb);
  // bwd_apply's blocks each sum the slices of their channels first (nsl x tw x V floats from L2):
  // 512 blocks keep that under a quarter of the stream's own bytes at B2 480 x 640
  const long want = ADD ? 512 : 2048;
  const long cap = want / ((long)ntile * B) > 0 ? want / ((long)ntile * B) : 1;
  if (nb > cap) nb = cap;
  CMX_DISPATCH(dtype, T, {
    hipLaunchKernelGGL((se_stream_kernel<T, ADD>), dim3((unsigned)nb, ntile, B), dim3(256), 0, s, (const T*)x, a,
                       dscale, part, nsl, ss, (T*)out, B, N, C, tw);
  });
  return cmx_check_launch(what);
}

}  // namespace

extern "C" {

int cmx_se_chunk_rows(void) { return SE_CHUNK; }

int cmx_se_pool_nchunk(int B, int N, int C) { return N > 0 ? se_nchunk(N) : 0; }

size_t cmx_se_pool_workspace(int B, int N, int C) {
  if (B <= 0 || N <= 0 || C <= 0) return 0;
  return (size_t)B * se_nchunk(N) * C * sizeof(float);
}

size_t cmx_se_pool_tickets(int B, int C) {
  if (B <= 0 || C <= 0 || C % 8) return 0;
  return (size_t)B * (C / pow2_div(C, SE_RED_CW));
}

int cmx_se_pool_fwd(const void* y, float* pooled, float* workspace, unsigned* tickets, int B, int N, int C, int dtype,
                    hipStream_t s) {
  CMX_REQUIRE(se_shape_ok(B, N, C), CMX_ERR_SHAPE, "se_pool_fwd: B=%d N=%d C=%d (C %% 8 == 0)", B, N, C);
  CMX_REQUIRE(y && pooled && workspace && tickets && al16(y), CMX_ERR_ARG,
              "se_pool_fwd: NULL or misaligned buffer (y on 16 B; caller-owned workspace and tickets)");
  const int cw = pow2_div(C, SE_RED_CW), nz = se_nchunk(N), chunk = (N + nz - 1) / nz;
  CMX_REQUIRE(C / cw <= 65535, CMX_ERR_SHAPE, "se_pool_fwd: C=%d has %d column tiles", C, C / cw);
  CMX_DISPATCH(dtype, T, {
    hipLaunchKernelGGL((se_reduce_kernel<T, false>), dim3(nz, C / cw, B), dim3(256), 0, s, (const T*)y,
                       (const T*)nullptr, (const float*)nullptr, workspace, pooled, tickets, B, N, C, cw, chunk);
  });
  return cmx_check_launch("se_pool_fwd");
}

int cmx_se_scale_fwd(const void* y, const float* a, const float* dscale, void* out, int B, int N, int C, int dtype,
                     hipStream_t s) {
  CMX_REQUIRE(se_shape_ok(B, N, C), CMX_ERR_SHAPE, "se_scale_fwd: B=%d N=%d C=%d (C %% 8 == 0)", B, N, C);
  CMX_REQUIRE(y && a && out && al16(y) && al16(a) && al16(dscale) && al16(out), CMX_ERR_ARG,
              "se_scale_fwd: NULL or misaligned buffer (16 B)");
  return se_stream<false>(y, a, dscale, nullptr, 0, 0, out, B, N, C, dtype, s, "se_scale_fwd");
}

int cmx_se_bwd_nslice(int B, int N, int C) { return N > 0 ? se_nchunk(N) : 0; }

int cmx_se_bwd_reduce(const void* dout, const void* y, const float* dscale, float* da_part, int B, int N, int C,
                      int dtype, hipStream_t s) {
  CMX_REQUIRE(se_shape_ok(B, N, C), CMX_ERR_SHAPE, "se_bwd_reduce: B=%d N=%d C=%d (C %% 8 == 0)", B, N, C);
  CMX_REQUIRE(dout && y && da_part && al16(dout) && al16(y), CMX_ERR_ARG,
              "se_bwd_reduce: NULL or misaligned buffer (16 B)");
  const int cw = pow2_div(C, SE_RED_CW), nz = se_nchunk(N), chunk = (N + nz - 1) / nz;
  CMX_REQUIRE(C / cw <= 65535, CMX_ERR_SHAPE, "se_bwd_reduce: C=%d has %d column tiles", C, C / cw);
  CMX_DISPATCH(dtype, T, {
    hipLaunchKernelGGL((se_reduce_kernel<T, true>), dim3(nz, C / cw, B), dim3(256), 0, s, (const T*)y, (const T*)dout,
                       dscale, da_part, (float*)nullptr, (unsigned*)nullptr, B, N, C, cw, chunk);
  });
  return cmx_check_launch("se_bwd_reduce");
}

int cmx_se_bwd_apply(const void* dout, const float* a, const float* dscale, const float* dpool_part, int nslice,
                     int64_t slice_stride, void* dy, int B, int N, int C, int dtype, hipStream_t s) {
  CMX_REQUIRE(se_shape_ok(B, N, C) && nslice > 0 && nslice <= SE_SL_MAX && slice_stride % 4 == 0 && slice_stride >= 0,
              CMX_ERR_SHAPE, "se_bwd_apply: B=%d N=%d C=%d nslice=%d (<= %d) slice_stride=%ld", B, N, C, nslice,
              SE_SL_MAX, (long)slice_stride);
  CMX_REQUIRE(dout && a && dpool_part && dy && al16(dout) && al16(a) && al16(dscale) && al16(dpool_part) && al16(dy),
              CMX_ERR_ARG, "se_bwd_apply: NULL or misaligned buffer (16 B)");
  return se_stream<true>(dout, a, dscale, dpool_part, nslice, (long)slice_stride, dy, B, N, C, dtype, s,
                         "se_bwd_apply");
}

}  // extern "C"
