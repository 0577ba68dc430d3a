// Final upsample + ProbOhemCrossEntropy2d (utils/loss_opr.py:205-255; the math is stated at the top of
// loss_cells.h).  The threshold is a global order statistic of the valid pixels' target-class
// probability, known only after every pixel was seen, so the forward is a sequence of launches, none of
// which materialises a full-resolution K-channel tensor or reads anything back to the host:
//   1. ohem_zero_kernel: the select's workspace (two counters, three histograms) zeroed
//   2. loss_cells<LK_OSTAT>: py (B, H, W) fp32 and the integer counts n_valid, n_below (p_y <= thresh)
//   3. ohem_hist_kernel<0..2>: an exact radix select of the min_kept-th smallest py on its bit pattern
//      (a non-negative float orders as its uint32), digits of 11, 11 and 10 bits from the top; each pass
//      builds the histogram of its digit over the keys that carry the digits chosen so far, privatised
//      in LDS and merged with integer atomics.  Each pass re-derives the earlier passes' choice from
//      their finished histograms; when the k-th value is not needed (nothing dropped, or n_below >=
//      min_kept: the threshold is thresh) every pass returns at once -- decided on the device
//   4. ohem_final_kernel: threshold and counts = [n_valid, n_below, n_kept]
//   5. loss_cells<LK_OHEM>: LK_CE's forward with the pixels whose py exceeds the threshold ignored
//   6. loss_finalize_kernel: out = [loss, 1 / n_kept, n_kept]
// Every dependency between blocks is a kernel boundary: no flag, ticket or spin wait, every loop bounded
// at launch.  The only atomics are integer adds, so every result is bit-identical from run to run.
#include "loss_cells.h"
#include "../../include/cmx_ohem.h"  // compiler-checks the definitions below against the ABI header

namespace {

constexpr int OS_NT = 256;
constexpr int OS_PASSES = 3;
constexpr unsigned OS_SENT_BITS = 0x40000000u;    // bits of OHEM_SENTINEL: a key at or above it is not valid
// workspace words: the two counters, then one histogram per pass
enum { OW_NVALID = 0, OW_NBELOW = 1, OW_HIST = 4, OW_HIST_STRIDE = 2048, OW_WORDS = OW_HIST + OS_PASSES * OW_HIST_STRIDE };

// pass p's digit is the key's bits [os_shift(p), os_shift(p) + log2 os_bins(p)): a bit-field, so every
// bit pattern (NaN included) indexes inside the histogram
__host__ __device__ constexpr int os_shift(int p) { return p == 0 ? 21 : p == 1 ? 10 : 0; }
__host__ __device__ constexpr int os_bins(int p) { return p == 2 ? 1024 : 2048; }
__host__ __device__ constexpr int os_hist(int p) { return OW_HIST + p * OW_HIST_STRIDE; }

// the k-th smallest is needed: something is dropped and thresh does not decide it.  ws's counters are
// complete before the launch that reads them, so the answer is the same in every block of every pass
__device__ __forceinline__ bool os_selects(const unsigned* ws, int min_kept) {
  return min_kept > 0 && (unsigned)min_kept <= ws[OW_NVALID] && ws[OW_NBELOW] < (unsigned)min_kept;
}

// Whole block: digit = the bin of hist (NB bins) that holds its k-th smallest entry (k from 1), krem =
// k's rank inside that bin.  sc: OS_NT + 2 words of LDS.  k above the histogram's total (no caller
// does that) gives the last bin, rank 1.
template <int NB>
__device__ void os_pick(const unsigned* __restrict__ hist, unsigned k, unsigned* sc, unsigned& digit, unsigned& krem) {
  constexpr int PER = NB / OS_NT;
  const int t = threadIdx.x;
  unsigned c[PER], s = 0;
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    c[i] = hist[t * PER + i];
    s += c[i];
  }
  sc[t] = s;
  if (t == 0) {
    sc[OS_NT] = NB - 1;
    sc[OS_NT + 1] = 1;
  }
  __syncthreads();
  for (int o = 1; o < OS_NT; o <<= 1) {           // inclusive scan of the threads' sums
    const unsigned v = t >= o ? sc[t - o] : 0u;
    __syncthreads();
    sc[t] += v;
    __syncthreads();
  }
  unsigned below = sc[t] - s;
  if (below < k && k <= sc[t]) {                  // one thread: the k-th lies in its bins
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      if (k > below && k <= below + c[i]) {
        sc[OS_NT] = t * PER + i;
        sc[OS_NT + 1] = k - below;
      }
      below += c[i];
    }
  }
  __syncthreads();
  digit = sc[OS_NT];
  krem = sc[OS_NT + 1];
  __syncthreads();                                // sc is free for the next pick
}

// The counters and histograms zeroed by a launch of their own: a kernel boundary, like every other
// dependency here
__global__ __launch_bounds__(OS_NT) void ohem_zero_kernel(unsigned* __restrict__ ws) {
  const int i = blockIdx.x * OS_NT + threadIdx.x;
  if (i < OW_WORDS) ws[i] = 0;
}

void ohem_zero_launch(unsigned* ws, hipStream_t s) {
  hipLaunchKernelGGL(ohem_zero_kernel, dim3((OW_WORDS + OS_NT - 1) / OS_NT), dim3(OS_NT), 0, s, ws);
}

// n_valid and n_below of keys that no statistics pass counted (cmx_ohem_select)
__global__ __launch_bounds__(OS_NT) void ohem_count_kernel(const float* __restrict__ py, long n, float thresh,
                                                           unsigned* __restrict__ ws) {
  __shared__ unsigned cnt[2];
  const int t = threadIdx.x;
  if (t < 2) cnt[t] = 0;
  __syncthreads();
  unsigned nv = 0, nb = 0;
  for (long i = (long)blockIdx.x * OS_NT + t; i < n; i += (long)gridDim.x * OS_NT) {
    const float p = py[i];
    if (__float_as_uint(p) < OS_SENT_BITS) {
      nv += 1;
      nb += p <= thresh ? 1 : 0;
    }
  }
  if (nv) atomicAdd(&cnt[0], nv);
  if (nb) atomicAdd(&cnt[1], nb);
  __syncthreads();
  if (t < 2 && cnt[t]) atomicAdd(&ws[t], cnt[t]);
}

template <int P>
__global__ __launch_bounds__(OS_NT) void ohem_hist_kernel(const float* __restrict__ py, long n, int min_kept,
                                                          unsigned* __restrict__ ws) {
  if (!os_selects(ws, min_kept)) return;
  __shared__ unsigned h[os_bins(P)];
  __shared__ unsigned sc[OS_NT + 2];
  const int t = threadIdx.x;
  // the digits chosen by the earlier passes, as the key's bits above this pass's digit
  unsigned prefix = 0, k = min_kept;
  if constexpr (P >= 1) {
    unsigned d, kr;
    os_pick<os_bins(0)>(ws + os_hist(0), k, sc, d, kr);
    prefix = d;
    k = kr;
  }
  if constexpr (P >= 2) {
    unsigned d, kr;
    os_pick<os_bins(1)>(ws + os_hist(1), k, sc, d, kr);
    prefix = prefix << 11 | d;
  }
  for (int i = t; i < os_bins(P); i += OS_NT) h[i] = 0;
  __syncthreads();
  for (long i = (long)blockIdx.x * OS_NT + t; i < n; i += (long)gridDim.x * OS_NT) {
    const unsigned u = __float_as_uint(py[i]);
    bool in = u < OS_SENT_BITS;
    if constexpr (P >= 1) in = in && (u >> os_shift(P - 1)) == prefix;
    if (in) atomicAdd(&h[(u >> os_shift(P)) & (os_bins(P) - 1)], 1u);
  }
  __syncthreads();
  for (int i = t; i < os_bins(P); i += OS_NT)
    if (h[i]) atomicAdd(&ws[os_hist(P) + i], h[i]);
}

// One block.  threshold and counts = [n_valid, n_below, n_kept]; n_kept counts every key <= threshold
// (ties at the k-th value are all kept)
__global__ __launch_bounds__(OS_NT) void ohem_final_kernel(float thresh, int min_kept, const unsigned* __restrict__ ws,
                                                           float* __restrict__ threshold, int64_t* __restrict__ counts) {
  __shared__ unsigned sc[OS_NT + 2];
  const unsigned nv = ws[OW_NVALID], nb = ws[OW_NBELOW];
  float thr;
  unsigned nk;
  if (os_selects(ws, min_kept)) {
    unsigned d0, d1, d2, k1, k2, k3;
    os_pick<os_bins(0)>(ws + os_hist(0), (unsigned)min_kept, sc, d0, k1);
    os_pick<os_bins(1)>(ws + os_hist(1), k1, sc, d1, k2);
    os_pick<os_bins(2)>(ws + os_hist(2), k2, sc, d2, k3);
    // n_below < min_kept: the k-th smallest exceeds thresh, so it is the threshold
    thr = __uint_as_float(d0 << os_shift(0) | d1 << os_shift(1) | d2);
    nk = (unsigned)min_kept - k3 + ws[os_hist(2) + d2];
  } else if (min_kept > 0 && (unsigned)min_kept <= nv) {
    thr = thresh;
    nk = nb;
  } else {                                        // nothing is dropped
    thr = INFINITY;
    nk = nv;
  }
  if (threadIdx.x == 0) {
    threshold[0] = thr;
    counts[0] = nv;
    counts[1] = nb;
    counts[2] = nk;
  }
}

// counted: ws's counters were filled by the statistics pass.  ws was zeroed (ohem_zero_launch) before that.
void ohem_select_launch(const float* py, long n, float thresh, int min_kept, bool counted, float* threshold,
                        int64_t* counts, unsigned* ws, hipStream_t s) {
  const long want = (n + 16 * OS_NT - 1) / (16 * OS_NT);     // 16 keys a thread, 256 blocks at the most
  const int grid = (int)(want < 256 ? want : 256);
  if (!counted) hipLaunchKernelGGL(ohem_count_kernel, dim3(grid), dim3(OS_NT), 0, s, py, n, thresh, ws);
  hipLaunchKernelGGL(ohem_hist_kernel<0>, dim3(grid), dim3(OS_NT), 0, s, py, n, min_kept, ws);
  hipLaunchKernelGGL(ohem_hist_kernel<1>, dim3(grid), dim3(OS_NT), 0, s, py, n, min_kept, ws);
  hipLaunchKernelGGL(ohem_hist_kernel<2>, dim3(grid), dim3(OS_NT), 0, s, py, n, min_kept, ws);
  hipLaunchKernelGGL(ohem_final_kernel, dim3(1), dim3(OS_NT), 0, s, thresh, min_kept, ws, threshold, counts);
}

constexpr size_t OS_WS_BYTES = (size_t)OW_WORDS * sizeof(unsigned);

}  // namespace

extern "C" {

size_t cmx_ohem_select_workspace(int64_t n) { return n > 0 && n <= INT32_MAX ? OS_WS_BYTES : 0; }

int cmx_ohem_select(const float* py, int64_t n, float thresh, int min_kept, float* threshold, int64_t* counts,
                    void* workspace, hipStream_t s) {
  CMX_REQUIRE(n > 0 && n <= INT32_MAX, CMX_ERR_ARG, "ohem_select: needs 0 < n < 2^31 (n=%lld)", (long long)n);
  CMX_REQUIRE(thresh == thresh, CMX_ERR_ARG, "ohem_select: thresh is NaN");
  CMX_REQUIRE(py && threshold && counts && workspace, CMX_ERR_ARG, "ohem_select: null operand");
  ohem_zero_launch((unsigned*)workspace, s);
  ohem_select_launch(py, n, thresh, min_kept, false, threshold, counts, (unsigned*)workspace, s);
  return cmx_check_launch("ohem_select");
}

size_t cmx_upsample_ohem_workspace(int B, int h, int w) {
  if (B <= 0 || h <= 0 || w <= 0) return 0;
  return OS_WS_BYTES + (size_t)loss_cells_nblk(B, h, w) * 2 * sizeof(float);
}

int cmx_upsample_ohem_fwd_adj(const void* logits, const int64_t* label, float* adj, float* out, float* py,
                              int64_t* counts, void* workspace, int B, int h, int w, int H, int W, int K,
                              int ignore_index, float thresh, int min_kept, int dtype, hipStream_t s) {
  CMX_REQUIRE(B > 0 && h > 0 && w > 0 && ce_tiled_ok(h, w, H, W, K), CMX_ERR_SHAPE,
              "upsample_ohem_fwd_adj: needs H = 4h, W = 4w, K <= %d (K=%d, %dx%d -> %dx%d)", KF, K, h, w, H, W);
  CMX_REQUIRE((int64_t)B * H * W <= INT32_MAX, CMX_ERR_SHAPE, "upsample_ohem_fwd_adj: %d x %d x %d pixels >= 2^31", B, H,
              W);
  CMX_REQUIRE(thresh == thresh, CMX_ERR_ARG, "upsample_ohem_fwd_adj: thresh is NaN");
  CMX_REQUIRE(dtype >= 0 && dtype <= 2, CMX_ERR_DTYPE, "upsample_ohem_fwd_adj: unsupported dtype %d", dtype);
  CMX_REQUIRE(logits && label && adj && out && py && counts && workspace, CMX_ERR_ARG,
              "upsample_ohem_fwd_adj: null operand");
  const int nb = loss_cells_nblk(B, h, w);
  unsigned* sel = (unsigned*)workspace;
  float* part = (float*)((char*)workspace + OS_WS_BYTES);
  float* threshold = out + 3;
  ohem_zero_launch(sel, s);
  CMX_DISPATCH(dtype, T, {
    loss_cells_launch<T, LK_OSTAT, 0, true>((const T*)logits, label, nullptr, nullptr, nullptr, py, (float*)sel, B, h, w,
                                            H, W, K, ignore_index, thresh, 0.f, 0.f, 0.f, s);
  });
  ohem_select_launch(py, (long)B * H * W, thresh, min_kept, true, threshold, counts, sel, s);
  CMX_DISPATCH(dtype, T, {
    loss_cells_launch<T, LK_OHEM, 0, true>((const T*)logits, label, py, nullptr, threshold, adj, part, B, h, w, H, W, K,
                                           ignore_index, 0.f, 0.f, 0.f, 0.f, s);
  });
  hipLaunchKernelGGL(loss_finalize_kernel<false>, dim3(1), dim3(256), 0, s, part, nb, out);
  return cmx_check_launch("upsample_ohem_fwd_adj");
}

}  // extern "C"
