// SRA attention, bf16 / head dim 64 fast path (every stage of CMX-B2/B4 at 480x640: Nk = 300).
//
// Same math as sra_attention.hip (dual_segformer.py:130-134: softmax(q k^T d^-1/2) v and its
// backward), re-decomposed for gfx950 around one fact: a whole (b, head)'s keys fit in LDS.
// K and V of one (b, head) are (Nk x 64) bf16 = 38 KB each at Nk = 300, so a workgroup
// stages BOTH once, in its prologue, and its waves then sweep every key tile with no
// barrier in the loop (the generic kernels restage a 32-key tile between two barriers per
// step, which left the stage-1 forward at ~4 % of MFMA peak).  80 KB of LDS per workgroup
// (Nk <= 320) keeps two workgroups per CU.
//
// Images: a key-row-major [nkp][64] bf16 image (128-B rows) per operand, 16-B chunks
// XOR-swizzled by (row >> 1) & 7.  A wave reads it two ways without a second copy:
//  * frag_k: 32 rows x 8 contiguous d per lane (ds_read_b128) -- K or V as the A operand of
//    S^T = K Q^T and dP^T = V dO^T;
//  * frag_t: the transposed view (d on the lane, 8 keys per lane) with gfx950's
//    ds_read_b64_tr_b16, in the k-permuted order in which an accumulator tile is fed back as
//    the B operand (accrow(8s + j, h), cmx_mfma.h) -- V^T of O^T = V^T P^T and K^T of
//    dQ^T = K^T dS^T, straight from the accumulator with no LDS round trip.
// Queries stay on the MFMA lane (S^T tiles), so the online softmax is per lane plus one
// cross-half shuffle; each wave owns QW 32-query sub-tiles for MFMA/VALU overlap.
//
// Shared __forceinline__ blocks (first section; the accumulator store is cmx_mfma.h's): the score mask
// and row max of the forwards, and for the short-sequence kernels the K / V staging, the dQ row
// prologue, the dQ dS tile and the output sum.  The three fast kernels keep their own offset tables,
// tile driver, staging, row prologues and dS block, both forwards their exponent loop and both
// dK / dV kernels their P / dS block: each of those, moved into a helper, changed a fast kernel's
// register allocation (sra_fwd_fast measured slower for it) or, in the dK / dV kernels, which product
// of S sl2 - lse log2 e the compiler fuses, and with it result bits (profiles/sra_dedupe/README.md).
#include "cmx_dma.h"
#include "cmx_mfma.h"
#include "sra_args.h"
#include <stdlib.h>

namespace {

template <typename E> using frag8 = typename MF<E>::frag;


typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef float f2 __attribute__((ext_vector_type(2)));     // packed fp32 pair (v_pk_fma / add / mul)

constexpr int HD = 64;          // head dim
constexpr int ROWB = 128;       // bytes per key row of an image
constexpr int NKP_MAX = 320;    // keys held in LDS (Nk <= 320)
constexpr int KTILE = 64;       // keys per loop step
constexpr int NWAVE = 8;        // waves per workgroup: two per SIMD share one K/V image

__device__ __forceinline__ int swz(int row) { return (row >> 1) & 7; }

// rows [0, nkp) of a (Nk x 64) bf16 matrix with row stride ld -> swizzled image, by LDS-DMA
// (no register staging; rows >= Nk come back as zeros through the buffer range check).  One
// wave instruction fills 8 rows (1 KB) in lane order: lane L lands on row 8j + L / 8, slot
// L % 8, which must hold chunk (L % 8) ^ swz(row).  Completion: vm_wait<0>() + barrier.
template <typename E>
__device__ __forceinline__ void stage_rows(const E* __restrict__ g, long ld, int Nk, int nkp, char* img, int wave,
                                           int lane, int nwaves) {
  const i32x4 rs = make_rsrc(g);
  for (int j = wave; j < nkp / 8; j += nwaves) {
    const int row = j * 8 + (lane >> 3), c = (lane & 7) ^ swz(row);
    const int off = row < Nk ? (int)(((long)row * ld + c * 8) * 2) : OOB;
    dma16(rs, lds_addr(img + j * 1024), off);
  }
}

// keys [r0, r0 + n) of (b, head): K -> image Ki, V -> image Vi (nkp rows each, zero past n), issued by
// `nwaves` waves (this one is `wave`); the caller waits
template <typename E>
__device__ __forceinline__ void stage_kv(const E* k, const E* v, int b, int head, int Nk, long kvs, int r0, int n,
                                         int nkp, char* Ki, char* Vi, int wave, int lane, int nwaves) {
  stage_rows(k + ((long)b * Nk + r0) * kvs + head * HD, kvs, n, nkp, Ki, wave, lane, nwaves);
  stage_rows(v + ((long)b * Nk + r0) * kvs + head * HD, kvs, n, nkp, Vi, wave, lane, nwaves);
}

// A operand, k = d contiguous: row rb + (lane & 31), d in [16 s + 8 h, +8)
template <typename E>
__device__ __forceinline__ frag8<E> frag_k(const char* img, int rb, int s, int lane) {
  const int row = rb + (lane & 31), h = lane >> 5;
  return frag_bits<E>(*reinterpret_cast<const uint4*>(img + row * ROWB + (((2 * s + h) ^ swz(row)) << 4)));
}

// A operand from the transposed view: d = db + (lane & 31) on the lane, k = rows
// kb + 16 s + 4 h + {0..3, 8..11} (the accumulator-as-B order of MF<E>::from_acc)
template <typename E>
__device__ __forceinline__ frag8<E> frag_t(const char* img, int kb, int db, int s, int lane) {
  const int h = lane >> 5, g16 = (lane >> 4) & 1, i = lane & 15, q = i >> 2, pp = i & 3;
  const int chunk = (db + 16 * g16 + 4 * pp) >> 3;
  s16x4 v[2];
#pragma unroll
  for (int rd = 0; rd < 2; ++rd) {
    const int kk = kb + 16 * s + 4 * h + 8 * rd + q;
    const int off = kk * ROWB + ((chunk ^ swz(kk)) << 4) + ((pp & 1) << 3);
    v[rd] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        reinterpret_cast<__attribute__((address_space(3))) s16x4*>(reinterpret_cast<uintptr_t>(img + off)));
  }
  const s16x8 c = __builtin_shufflevector(v[0], v[1], 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(frag8<E>, c);
}

// The same reads with the per-lane part of the address precomputed once per kernel: with row
// bases that are multiples of 16 the swizzle depends only on the lane, so a tile's address is
// (uniform tile base) + (per-lane offset) + (compile-time sub-tile offset).  A runtime key loop
// then costs one add per distinct per-lane offset per tile instead of a full recomputation.
__device__ __forceinline__ int koff(int s, int lane) {
  const int row = lane & 31, h = lane >> 5;
  return row * ROWB + (((2 * s + h) ^ swz(row)) << 4);
}
__device__ __forceinline__ int toff(int rd, int db, int lane) {
  const int h = lane >> 5, g16 = (lane >> 4) & 1, i = lane & 15, q = i >> 2, pp = i & 3;
  const int chunk = (db + 16 * g16 + 4 * pp) >> 3, kk = 4 * h + 8 * rd + q;
  return kk * ROWB + ((chunk ^ swz(kk)) << 4) + ((pp & 1) << 3);
}
template <typename E>
__device__ __forceinline__ frag8<E> frag_k_o(const char* p) {
  return frag_bits<E>(*reinterpret_cast<const uint4*>(p));
}
template <typename E>
__device__ __forceinline__ frag8<E> frag_t_o(const char* p0, const char* p1) {
  const s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      reinterpret_cast<__attribute__((address_space(3))) s16x4*>(reinterpret_cast<uintptr_t>(p0)));
  const s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      reinterpret_cast<__attribute__((address_space(3))) s16x4*>(reinterpret_cast<uintptr_t>(p1)));
  return __builtin_bit_cast(frag8<E>, __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7));
}

__device__ __forceinline__ float fexp2(float x) { return __builtin_amdgcn_exp2f(x); }

// ---- the forwards: mask and row max on the raw S^T scores of one 64-key tile (query on the lane)
// keys >= nk of the tile at key t0 score -inf
__device__ __forceinline__ void mask_scores(f32x16 (&sa)[2], int t0, int nk, int h) {
#pragma unroll
  for (int ks = 0; ks < 2; ++ks)
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (t0 + 32 * ks + accrow(i, h) >= nk) sa[ks][i] = -INFINITY;
}
// the row max in log2 units: max on the raw scores (the scale is positive)
__device__ __forceinline__ float score_max(const f32x16 (&sa)[2], float sl2) {
  float mt = -INFINITY;
#pragma unroll
  for (int ks = 0; ks < 2; ++ks)
#pragma unroll
    for (int i = 0; i < 16; ++i) mt = fmaxf(mt, sa[ks][i]);
  return fmaxf(mt, xor_lane<32>(mt)) * sl2;
}

// ---- dQ, short sequences: the row prologue.  Query row qi of (b, head) on the lane (half h supplies its 8 elements of
// every k-step): the Q and dO fragments (zero past N), Dq = rowsum(dO . O) as one sum chained through
// the row, lse in log2 units; the `writer` lanes store Dq to Dws
template <typename E>
__device__ __forceinline__ void sra_dq_row(const E* q, const E* o, const E* dout, const float* lse, float* Dws, int b,
                                           int head, int heads, int N, int qi, long qs, long os, long dos, int h,
                                           bool writer, frag8<E> (&qf)[4], frag8<E> (&df)[4], float& Dq, float& lse2) {
  const bool live = qi < N;
  const E* qrow = q + ((long)b * N + qi) * qs + head * HD;
  const E* orow = o + ((long)b * N + qi) * os + head * HD;
  const E* drow = dout + ((long)b * N + qi) * dos + head * HD;
  float dot = 0.f;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    if (live) {
      qf[s] = frag_bits<E>(*reinterpret_cast<const uint4*>(qrow + 16 * s + 8 * h));
      df[s] = frag_bits<E>(*reinterpret_cast<const uint4*>(drow + 16 * s + 8 * h));
      float x[8], y[8];
      load_vec<E>(drow + 16 * s + 8 * h, x);
      load_vec<E>(orow + 16 * s + 8 * h, y);
#pragma unroll
      for (int j = 0; j < 8; ++j) dot += x[j] * y[j];
    } else {
      qf[s] = df[s] = zfrag<E>();
    }
  }
  dot += xor_lane<32>(dot);
  Dq = dot;
  const long sidx = ((long)b * heads + head) * N + qi;
  lse2 = live ? lse[sidx] * 1.4426950408889634f : 0.f;
  if (live && writer) Dws[sidx] = dot;
}

// ---- dQ, short sequences: dS^T of one 32-key x 32-query tile (query on the lane, keys kb + accrow(i, h)):
// p = exp2(S sl2 - lse2), p = 0 at keys >= nk, dS = p (dP - Dq) -> ds (which may be sa: each pair is
// read before it is written).  `ragged` (wave-uniform): the tile holds keys >= nk, the last wave's only
__device__ __forceinline__ void dq_ds_tile(const f32x16& sa, const f32x16& dp, f32x16& ds, float sl2, float lse2,
                                           float Dq, int kb, int nk, int h, bool ragged) {
  const f2 sl2v = {sl2, sl2}, nl = {-lse2, -lse2}, nD = {-Dq, -Dq};
#pragma unroll
  for (int i = 0; i < 16; i += 2) {
    const f2 a = f2{sa[i], sa[i + 1]} * sl2v + nl;
    f2 p = {fexp2(a.x), fexp2(a.y)};
    if (ragged) {
      if (kb + accrow(i, h) >= nk) p.x = 0.f;
      if (kb + accrow(i + 1, h) >= nk) p.y = 0.f;
    }
    const f2 d = p * (f2{dp[i], dp[i + 1]} + nD);
    ds[i] = d.x;
    ds[i + 1] = d.y;
  }
}

// ------------------------------------------------------------------------ forward
template <typename E, int QW, int NW>
__global__ __launch_bounds__(64 * NW) void sra_fwd_fast(const E* __restrict__ q, const E* __restrict__ k,
                                                       const E* __restrict__ v, E* __restrict__ o,
                                                       float* __restrict__ lse, int N, int Nk, int nkp, int heads,
                                                       long qs, long kvs, long os, float sl2) {
  __shared__ __attribute__((aligned(1024))) char smem[2 * NKP_MAX * ROWB];
  char* Ki = smem;
  char* Vi = smem + NKP_MAX * ROWB;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int b = blockIdx.z, head = blockIdx.y;

  const int q0 = (blockIdx.x * NW + wave) * 32 * QW;
  const E* qb = q + (long)b * N * qs + head * HD;
  frag8<E> qf[QW][4];
#pragma unroll
  for (int u = 0; u < QW; ++u) {
    const int qi = q0 + 32 * u + r;
#pragma unroll
    for (int s = 0; s < 4; ++s)
      qf[u][s] = qi < N ? frag_bits<E>(*reinterpret_cast<const uint4*>(qb + (long)qi * qs + 16 * s + 8 * h))
                        : zfrag<E>();
  }
  f32x16 acc[QW][2];
  float m[QW], l[QW];
#pragma unroll
  for (int u = 0; u < QW; ++u) {
    acc[u][0] = acc[u][1] = zero16();
    m[u] = -INFINITY;
    l[u] = 0.f;
  }
  // keys in LDS-sized chunks (one chunk when Nk <= NKP_MAX, every B2 / B4 stage; B5 at
  // 1024 x 1024 has Nk = 1024 at every stage): the online softmax state carries across chunks
  for (int c0 = 0; c0 < Nk; c0 += NKP_MAX) {
  const int nc = min(NKP_MAX, Nk - c0);
  const int nkc = (nc + KTILE - 1) / KTILE * KTILE;
  if (c0 > 0) __syncthreads();                  // every wave is done with the previous chunk
  stage_rows(k + ((long)b * Nk + c0) * kvs + head * HD, kvs, nc, nkc, Ki, wave, lane, NW);
  stage_rows(v + ((long)b * Nk + c0) * kvs + head * HD, kvs, nc, nkc, Vi, wave, lane, NW);
  vm_wait<0>();
  __syncthreads();

  // whole key tiles, then the ragged tail tile with the key mask: the unmasked tiles carry no
  // per-score compare / select
  int ko[4], to[2][2];
#pragma unroll
  for (int s = 0; s < 4; ++s) ko[s] = koff(s, lane);
#pragma unroll
  for (int rd = 0; rd < 2; ++rd)
#pragma unroll
    for (int d = 0; d < 2; ++d) to[rd][d] = toff(rd, 32 * d, lane);
  auto tile = [&](const int t0, auto masked) {
    constexpr bool MASK = decltype(masked)::value;
    const char* Kt = Ki + t0 * ROWB;
    const char* Vt = Vi + t0 * ROWB;
    f32x16 sa[QW][2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      frag8<E> kf[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) kf[s] = frag_k_o<E>(Kt + 32 * ks * ROWB + ko[s]);
#pragma unroll
      for (int u = 0; u < QW; ++u) {
        sa[u][ks] = zero16();
#pragma unroll
        for (int s = 0; s < 4; ++s) sa[u][ks] = MF<E>::mma(kf[s], qf[u][s], sa[u][ks]);
      }
    }
#pragma unroll
    for (int u = 0; u < QW; ++u) {
      if constexpr (MASK) mask_scores(sa[u], t0, nc, h);
      const float mt = score_max(sa[u], sl2);
      const float mn = fmaxf(m[u], mt);
      const float alpha = fexp2(m[u] - mn);
      const f2 sl2v = {sl2, sl2}, nmn = {-mn, -mn};
      f2 rs2 = {0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int i = 0; i < 16; i += 2) {
          const f2 x = {sa[u][ks][i], sa[u][ks][i + 1]};
          const f2 a = x * sl2v + nmn;
          const f2 p = {fexp2(a.x), fexp2(a.y)};
          sa[u][ks][i] = p.x;
          sa[u][ks][i + 1] = p.y;
          rs2 += p;
        }
      float rs = rs2.x + rs2.y;
      rs += xor_lane<32>(rs);
      l[u] = l[u] * alpha + rs;
      // rescale the accumulator only when some lane's running max moved: alpha == 1 exactly
      // otherwise, and after the first key tiles the max rarely moves
      if (__builtin_amdgcn_ballot_w64(mn != m[u])) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int i = 0; i < 16; ++i) acc[u][t][i] *= alpha;
      }
      m[u] = mn;
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const char* vp = Vt + (32 * ks + 16 * s) * ROWB;
        const frag8<E> v0 = frag_t_o<E>(vp + to[0][0], vp + to[1][0]);
        const frag8<E> v1 = frag_t_o<E>(vp + to[0][1], vp + to[1][1]);
#pragma unroll
        for (int u = 0; u < QW; ++u) {
          const frag8<E> pf = MF<E>::from_acc(sa[u][ks], s);
          acc[u][0] = MF<E>::mma(v0, pf, acc[u][0]);
          acc[u][1] = MF<E>::mma(v1, pf, acc[u][1]);
        }
      }
  };
  const int nfull = nc / KTILE;
  for (int t0 = 0; t0 < nfull * KTILE; t0 += KTILE) tile(t0, std::false_type{});
  if (nfull * KTILE < nc) tile(nfull * KTILE, std::true_type{});
  }                                             // key chunks
#pragma unroll
  for (int u = 0; u < QW; ++u) {
    const int qi = q0 + 32 * u + r;
    if (qi >= N) continue;
    const float inv = 1.f / l[u];
    E* ob = o + ((long)b * N + qi) * os + head * HD;
    store_acc_row(ob, acc[u][0], 0, h, inv);
    store_acc_row(ob, acc[u][1], 1, h, inv);
    if (h == 0 && lse) lse[((long)b * heads + head) * N + qi] = (m[u] + __log2f(l[u])) * 0.69314718055994531f;
  }
}

// ------------------------------------------------------------------------ backward: dQ (+ Dq)
// dS^T = P^T o (dP^T - Dq), P^T = exp(S^T - lse), dP^T = V dO^T; dQ^T = K^T dS^T * scale.
template <typename E, int QW, int NW>
__global__ __launch_bounds__(64 * NW) void sra_dq_fast(const E* __restrict__ q, const E* __restrict__ k,
                                                      const E* __restrict__ v, const E* __restrict__ o,
                                                      const E* __restrict__ dout, const float* __restrict__ lse,
                                                      float* __restrict__ Dws, E* __restrict__ dq, int N, int Nk,
                                                      int nkp, int heads, long qs, long kvs, long os, long dos,
                                                      long dqs, float sl2, float scale) {
  __shared__ __attribute__((aligned(1024))) char smem[2 * NKP_MAX * ROWB];
  char* Ki = smem;
  char* Vi = smem + NKP_MAX * ROWB;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int b = blockIdx.z, head = blockIdx.y;

  const int q0 = (blockIdx.x * NW + wave) * 32 * QW;
  frag8<E> qf[QW][4], df[QW][4];
  float Dq[QW], lse2[QW];
#pragma unroll
  for (int u = 0; u < QW; ++u) {
    const int qi = q0 + 32 * u + r;
    const bool live = qi < N;
    const E* qrow = q + ((long)b * N + qi) * qs + head * HD;
    const E* orow = o + ((long)b * N + qi) * os + head * HD;
    const E* drow = dout + ((long)b * N + qi) * dos + head * HD;
    float dot = 0.f;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      if (live) {
        const uint4 qv = *reinterpret_cast<const uint4*>(qrow + 16 * s + 8 * h);
        const uint4 dv = *reinterpret_cast<const uint4*>(drow + 16 * s + 8 * h);
        qf[u][s] = frag_bits<E>(qv);
        df[u][s] = frag_bits<E>(dv);
        float x[8], y[8];
        load_vec<E>(drow + 16 * s + 8 * h, x);
        load_vec<E>(orow + 16 * s + 8 * h, y);
#pragma unroll
        for (int j = 0; j < 8; ++j) dot += x[j] * y[j];
      } else {
        qf[u][s] = df[u][s] = zfrag<E>();
      }
    }
    dot += xor_lane<32>(dot);
    Dq[u] = dot;
    const long sidx = ((long)b * heads + head) * N + qi;
    lse2[u] = live ? lse[sidx] * 1.4426950408889634f : 0.f;
    if (live && h == 0) Dws[sidx] = dot;
  }
  f32x16 acc[QW][2];
#pragma unroll
  for (int u = 0; u < QW; ++u) acc[u][0] = acc[u][1] = zero16();
  // keys in LDS-sized chunks, as the forward (dQ sums over every key: nothing to carry but acc)
  for (int c0 = 0; c0 < Nk; c0 += NKP_MAX) {
  const int nc = min(NKP_MAX, Nk - c0);
  const int nkc = (nc + KTILE - 1) / KTILE * KTILE;
  if (c0 > 0) __syncthreads();                  // every wave is done with the previous chunk
  stage_rows(k + ((long)b * Nk + c0) * kvs + head * HD, kvs, nc, nkc, Ki, wave, lane, NW);
  stage_rows(v + ((long)b * Nk + c0) * kvs + head * HD, kvs, nc, nkc, Vi, wave, lane, NW);
  vm_wait<0>();
  __syncthreads();

  // whole key tiles, then the masked tail tile (see the forward)
  int ko[4], to[2][2];
#pragma unroll
  for (int s = 0; s < 4; ++s) ko[s] = koff(s, lane);
#pragma unroll
  for (int rd = 0; rd < 2; ++rd)
#pragma unroll
    for (int d = 0; d < 2; ++d) to[rd][d] = toff(rd, 32 * d, lane);
  auto tile = [&](const int t0, auto masked) {
    constexpr bool MASK = decltype(masked)::value;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int kb = t0 + 32 * ks;
      const char* Kt = Ki + kb * ROWB;
      const char* Vt = Vi + kb * ROWB;
      frag8<E> kf[4], vf[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        kf[s] = frag_k_o<E>(Kt + ko[s]);
        vf[s] = frag_k_o<E>(Vt + ko[s]);
      }
      f32x16 ds[QW];
#pragma unroll
      for (int u = 0; u < QW; ++u) {
        f32x16 sa = zero16(), dp = zero16();
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          sa = MF<E>::mma(kf[s], qf[u][s], sa);
          dp = MF<E>::mma(vf[s], df[u][s], dp);
        }
        const f2 sl2v = {sl2, sl2}, nl = {-lse2[u], -lse2[u]}, nD = {-Dq[u], -Dq[u]};
#pragma unroll
        for (int i = 0; i < 16; i += 2) {
          const f2 a = f2{sa[i], sa[i + 1]} * sl2v + nl;
          f2 p = {fexp2(a.x), fexp2(a.y)};
          if constexpr (MASK) {
            if (kb + accrow(i, h) >= nc) p.x = 0.f;
            if (kb + accrow(i + 1, h) >= nc) p.y = 0.f;
          }
          const f2 d = p * (f2{dp[i], dp[i + 1]} + nD);
          ds[u][i] = d.x;
          ds[u][i + 1] = d.y;
        }
      }
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const char* kp = Kt + 16 * s * ROWB;
        const frag8<E> k0 = frag_t_o<E>(kp + to[0][0], kp + to[1][0]);
        const frag8<E> k1 = frag_t_o<E>(kp + to[0][1], kp + to[1][1]);
#pragma unroll
        for (int u = 0; u < QW; ++u) {
          const frag8<E> sf = MF<E>::from_acc(ds[u], s);
          acc[u][0] = MF<E>::mma(k0, sf, acc[u][0]);
          acc[u][1] = MF<E>::mma(k1, sf, acc[u][1]);
        }
      }
    }
  };
  const int nfull = nc / KTILE;
  for (int t0 = 0; t0 < nfull * KTILE; t0 += KTILE) tile(t0, std::false_type{});
  if (nfull * KTILE < nc) tile(nfull * KTILE, std::true_type{});
  }                                             // key chunks
#pragma unroll
  for (int u = 0; u < QW; ++u) {
    const int qi = q0 + 32 * u + r;
    if (qi >= N) continue;
    E* out = dq + ((long)b * N + qi) * dqs + head * HD;
    store_acc_row(out, acc[u][0], 0, h, scale);
    store_acc_row(out, acc[u][1], 1, h, scale);
  }
}


// ------------------------------------------------------------------------ backward: dK, dV
// Key on the lane: a workgroup owns ALL keys of one (b, head) (wave w: keys 64w .. 64w + 63,
// their K and V fragments in registers) and sweeps a chunk of queries in 64-query tiles.  The
// Q / dO tiles (+ lse, Dq) are staged ONCE per workgroup by LDS-DMA into a double buffer and
// shared by every wave (the generic kernel re-staged them per 128-key workgroup).  Per tile
// and key sub-tile: S and dP (8 MFMA), P and dS on the VALU, dV^T += dO^T P and
// dK^T += Q^T dS (8 MFMA, the accumulators fed back as B operands).  Partial dK / dV of the
// chunk go to the fp32 slab sra_dkv_reduce_kernel folds (same layout as the generic path).
__device__ __forceinline__ void dma4(const i32x4 rsrc, uint32_t lds, int voffset) {
  asm volatile("s_mov_b32 m0, %0\n\tbuffer_load_dword %1, %2, 0 offen lds"
               :: "s"(__builtin_amdgcn_readfirstlane(lds)), "v"(voffset), "s"(rsrc) : "memory");
}

constexpr int QT = 64;                          // queries per tile
constexpr int DKV_TILE_BYTES = 2 * QT * ROWB + 2 * QT * 4;   // Q, dO images + lse, Dq

template <typename E>
__global__ __launch_bounds__(64 * (NKP_MAX / 32)) void sra_dkv_fast(
    const E* __restrict__ q, const E* __restrict__ k, const E* __restrict__ v, const E* __restrict__ dout,
    const float* __restrict__ lse, const float* __restrict__ Dws, float* __restrict__ ws_dk, float* __restrict__ ws_dv,
    E* __restrict__ dk, E* __restrict__ dv, long dkvs,
    int Bt, int N, int Nk, int heads, long qs, long kvs, long dos, int QC, int nchunk, float sl2, float scale) {
  __shared__ __attribute__((aligned(1024))) char smem[2 * DKV_TILE_BYTES];
  const int nw = blockDim.x >> 6;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  // blockIdx.x = (key chunk, query chunk): a workgroup holds at most NKP_MAX keys on its lanes
  const int head = blockIdx.y, b = blockIdx.z, c = blockIdx.x % nchunk, kc0 = blockIdx.x / nchunk * NKP_MAX;
  const int qbeg = c * QC, qend = min(N, qbeg + QC);
  const long sbase = ((long)b * heads + head) * N;
  const i32x4 rq = make_rsrc(q + (long)b * N * qs + head * HD);
  const i32x4 rd = make_rsrc(dout + (long)b * N * dos + head * HD);
  const i32x4 rl = make_rsrc(lse + sbase);
  const i32x4 rD = make_rsrc(Dws + sbase);

  // DMA of query tile [q0, q0 + 64): 8 Q + 8 dO row-groups (1 KB each) + lse + Dq, round-robin
  auto issue = [&](int q0, char* buf) {
    for (int j = wave; j < 18; j += nw) {
      if (j < 16) {
        const int row = (j & 7) * 8 + (lane >> 3), cc = (lane & 7) ^ swz(row);
        const int gq = q0 + row;
        if (j < 8) {
          const int off = gq < qend ? (int)(((long)gq * qs + cc * 8) * 2) : OOB;
          dma16(rq, lds_addr(buf + j * 1024), off);
        } else {
          const int off = gq < qend ? (int)(((long)gq * dos + cc * 8) * 2) : OOB;
          dma16(rd, lds_addr(buf + QT * ROWB + (j - 8) * 1024), off);
        }
      } else {
        const int gq = q0 + lane;
        const int off = gq < qend ? gq * 4 : OOB;
        if (j == 16) dma4(rl, lds_addr(buf + 2 * QT * ROWB), off);
        else dma4(rD, lds_addr(buf + 2 * QT * ROWB + QT * 4), off);
      }
    }
  };

  // this wave's 32 keys: K, V fragments as B operands (k = d), lane = key
  const int key = kc0 + 32 * wave + r;
  frag8<E> kf[4], vf[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    if (key < Nk) {
      kf[s] = frag_bits<E>(*reinterpret_cast<const uint4*>(k + ((long)b * Nk + key) * kvs + head * HD + 16 * s + 8 * h));
      vf[s] = frag_bits<E>(*reinterpret_cast<const uint4*>(v + ((long)b * Nk + key) * kvs + head * HD + 16 * s + 8 * h));
    } else {
      kf[s] = vf[s] = zfrag<E>();
    }
  }
  f32x16 ak[2], av[2];
  ak[0] = ak[1] = av[0] = av[1] = zero16();

  if (qbeg < qend) issue(qbeg, smem);
  vm_wait<0>();
  __syncthreads();
  // only the ragged last query tile carries the per-score query mask
  int ko[4], to[2][2];
#pragma unroll
  for (int s = 0; s < 4; ++s) ko[s] = koff(s, lane);
#pragma unroll
  for (int rd = 0; rd < 2; ++rd)
#pragma unroll
    for (int d = 0; d < 2; ++d) to[rd][d] = toff(rd, 32 * d, lane);
  int cur = 0;
  auto qtile = [&](const int q0, auto masked) {
    constexpr bool MASK = decltype(masked)::value;
    if (q0 + QT < qend) issue(q0 + QT, smem + (cur ^ 1) * DKV_TILE_BYTES);
    const char* Qi = smem + cur * DKV_TILE_BYTES;
    const char* Di = Qi + QT * ROWB;
    const float* ls = reinterpret_cast<const float*>(Qi + 2 * QT * ROWB);
    const float* Ds = ls + QT;
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      const int qb = 32 * qt;
      f32x16 sa = zero16(), dp = zero16();
#pragma unroll
      for (int s = 0; s < 4; ++s) sa = MF<E>::mma(frag_k_o<E>(Qi + qb * ROWB + ko[s]), kf[s], sa);
#pragma unroll
      for (int s = 0; s < 4; ++s) dp = MF<E>::mma(frag_k_o<E>(Di + qb * ROWB + ko[s]), vf[s], dp);
      const f2 sl2v = {sl2, sl2}, nlog2e = {-1.4426950408889634f, -1.4426950408889634f};
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const float4 l4 = *reinterpret_cast<const float4*>(ls + qb + 8 * g4 + 4 * h);
        const float4 d4 = *reinterpret_cast<const float4*>(Ds + qb + 8 * g4 + 4 * h);
#pragma unroll
        for (int e = 0; e < 4; e += 2) {
          const int i = 4 * g4 + e;
          const f2 lv = e == 0 ? f2{l4.x, l4.y} : f2{l4.z, l4.w};
          const f2 dv = e == 0 ? f2{d4.x, d4.y} : f2{d4.z, d4.w};
          const f2 a = f2{sa[i], sa[i + 1]} * sl2v + lv * nlog2e;
          f2 p = {fexp2(a.x), fexp2(a.y)};
          if constexpr (MASK) {
            if (q0 + qb + accrow(i, h) >= qend) p.x = 0.f;
            if (q0 + qb + accrow(i + 1, h) >= qend) p.y = 0.f;
          }
          const f2 d = p * (f2{dp[i], dp[i + 1]} - dv);
          sa[i] = p.x; sa[i + 1] = p.y;
          dp[i] = d.x; dp[i + 1] = d.y;
        }
      }
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const frag8<E> pf = MF<E>::from_acc(sa, s);
        const frag8<E> sf = MF<E>::from_acc(dp, s);
        const char* dpp = Di + (qb + 16 * s) * ROWB;
        const char* qpp = Qi + (qb + 16 * s) * ROWB;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          av[t] = MF<E>::mma(frag_t_o<E>(dpp + to[0][t], dpp + to[1][t]), pf, av[t]);
          ak[t] = MF<E>::mma(frag_t_o<E>(qpp + to[0][t], qpp + to[1][t]), sf, ak[t]);
        }
      }
    }
    vm_wait<0>();
    __syncthreads();
    cur ^= 1;
  };
  const int nfull = (qend - qbeg) / QT;
  for (int q0 = qbeg; q0 < qbeg + nfull * QT; q0 += QT) qtile(q0, std::false_type{});
  if (qbeg + nfull * QT < qend) qtile(qbeg + nfull * QT, std::true_type{});
  if (key >= Nk) return;
  if (nchunk == 1) {            // one query chunk: this workgroup's sums are the gradients
    E* ok = dk + ((long)b * Nk + key) * dkvs + head * HD;
    E* ov = dv + ((long)b * Nk + key) * dkvs + head * HD;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int d = 32 * t + 8 * g4 + 4 * h;
        *reinterpret_cast<uint2*>(ok + d) = make_uint2(pack2<E>(ak[t][4 * g4] * scale, ak[t][4 * g4 + 1] * scale),
                                                       pack2<E>(ak[t][4 * g4 + 2] * scale, ak[t][4 * g4 + 3] * scale));
        *reinterpret_cast<uint2*>(ov + d) = make_uint2(pack2<E>(av[t][4 * g4], av[t][4 * g4 + 1]),
                                                       pack2<E>(av[t][4 * g4 + 2], av[t][4 * g4 + 3]));
      }
    return;
  }
  const long o = ((((long)c * Bt + b) * heads + head) * Nk + key) * HD;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const int d = 32 * t + 8 * g4 + 4 * h;
      *reinterpret_cast<float4*>(ws_dk + o + d) = make_float4(ak[t][4 * g4] * scale, ak[t][4 * g4 + 1] * scale,
                                                              ak[t][4 * g4 + 2] * scale, ak[t][4 * g4 + 3] * scale);
      *reinterpret_cast<float4*>(ws_dv + o + d) = make_float4(av[t][4 * g4], av[t][4 * g4 + 1], av[t][4 * g4 + 2],
                                                              av[t][4 * g4 + 3]);
    }
}

// ------------------------------------------------------------------------ short sequences
// Stages 3 / 4 of B2 / B4 (N = 1200 / 300 queries per (b, head), Nk = 300 keys): the kernels
// above stage all of a (b, head)'s keys in every workgroup and walk them serially, so with
// 64 queries per workgroup the K / V staging and the 5-step key loop are a latency chain the
// chip cannot fill (11-23 us per launch for 0.6-1.8 GFLOP).  Here the keys are split over the
// waves of a workgroup instead: wave w owns the w-th 64-key tile (its K / V image in its own
// LDS region, staged and read by that wave alone, so no barrier guards it), and the waves'
// partial results meet once in LDS at the end.  dK / dV keep the keys on the lanes and split
// the QUERY tiles over the waves, so every key's gradient is summed inside one workgroup: no
// partial slabs and no reduce launch.
constexpr int SKT = NKP_MAX / KTILE;           // key tiles of 64 (Nk <= 320): waves per workgroup
constexpr int SREG = 2 * KTILE * ROWB;          // per-wave LDS region: two 64-row images (16 KB)
constexpr int SQW = 8;                          // dK / dV: query-tile waves per workgroup
constexpr int SDREG = 2 * KTILE * ROWB + 2 * KTILE * 4;   // dK / dV region: Q, dO images + lse, Dq

// fp32 [row][64] tile in a wave's region, 16-B chunks XOR-swizzled by (row & 15): the lanes of
// one accumulator write (32 rows, one chunk each) spread over the bank row
__device__ __forceinline__ float* xrow(char* reg, int row, int chunk) {
  return reinterpret_cast<float*>(reg + row * 256 + ((chunk ^ (row & 15)) << 4));
}

// acc (lane = row r of the 32-row block rb, registers = 32 columns of column block 32 t) scaled
// by `mul` -> the wave's fp32 [row][64] tile
__device__ __forceinline__ void put_tile(char* reg, const f32x16& acc, int rb, int t, int lane, float mul) {
  const int r = lane & 31, h = lane >> 5, row = rb + r;
#pragma unroll
  for (int g4 = 0; g4 < 4; ++g4)
    *reinterpret_cast<float4*>(xrow(reg, row, 8 * t + 2 * g4 + h)) =
        make_float4(acc[4 * g4] * mul, acc[4 * g4 + 1] * mul, acc[4 * g4 + 2] * mul, acc[4 * g4 + 3] * mul);
}

// out row `row`, columns [8 dg, 8 dg + 8) = sum over the nw regions (stride `rs` bytes) * mul
template <typename E>
__device__ __forceinline__ void sum_store8(const char* smem, int nw, long rs, int row, int dg, float mul, E* out) {
  float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int w = 0; w < nw; ++w) {
    char* reg = const_cast<char*>(smem) + w * rs;
    const float4 x = *reinterpret_cast<const float4*>(xrow(reg, row, 2 * dg));
    const float4 y = *reinterpret_cast<const float4*>(xrow(reg, row, 2 * dg + 1));
    a[0] += x.x; a[1] += x.y; a[2] += x.z; a[3] += x.w; a[4] += y.x; a[5] += y.y; a[6] += y.z; a[7] += y.w;
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) a[e] *= mul;
  store_vec<E>(out, a);
}

// the end of the short-sequence forward and dQ: the waves' [rows][64] tiles (put_tile) summed into
// query rows [q0, q0 + rows) of (b, head) of `out` (row stride ld), rows past N left alone
template <typename E>
__device__ __forceinline__ void sum_store_queries(const char* smem, int nw, int rows, E* out, int b, int head, int N,
                                                  int q0, long ld) {
  __syncthreads();
  for (int it = threadIdx.x; it < rows * 8; it += blockDim.x) {
    const int row = it >> 3, dg = it & 7, qi = q0 + row;
    if (qi < N) sum_store8<E>(smem, nw, SREG, row, dg, 1.f, out + ((long)b * N + qi) * ld + head * HD + 8 * dg);
  }
}

// forward: workgroup = 64 queries of one (b, head); wave w = key tile w
template <typename E>
__global__ __launch_bounds__(64 * SKT) void sra_fwd_small(const E* __restrict__ q, const E* __restrict__ k,
                                                         const E* __restrict__ v, E* __restrict__ o,
                                                         float* __restrict__ lse, int N, int Nk, int heads, long qs,
                                                         long kvs, long os, float sl2) {
  __shared__ __attribute__((aligned(1024))) char smem[SKT * SREG];
  const int nw = blockDim.x >> 6;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int b = blockIdx.z, head = blockIdx.y, q0 = blockIdx.x * 64;
  char* Ki = smem + wave * SREG;
  char* Vi = Ki + KTILE * ROWB;
  const int t0 = wave * KTILE, nkw = min(KTILE, Nk - t0);
  stage_kv(k, v, b, head, Nk, kvs, t0, nkw, KTILE, Ki, Vi, 0, lane, 1);
  const E* qb = q + (long)b * N * qs + head * HD;
  frag8<E> qf[2][4];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int qi = q0 + 32 * u + r;
#pragma unroll
    for (int s = 0; s < 4; ++s)
      qf[u][s] = qi < N ? frag_bits<E>(*reinterpret_cast<const uint4*>(qb + (long)qi * qs + 16 * s + 8 * h)) : zfrag<E>();
  }
  vm_wait<0>();                                  // this wave's own images (no other wave reads them)
  f32x16 sa[2][2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    frag8<E> kf[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) kf[s] = frag_k<E>(Ki, 32 * ks, s, lane);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      sa[u][ks] = zero16();
#pragma unroll
      for (int s = 0; s < 4; ++s) sa[u][ks] = MF<E>::mma(kf[s], qf[u][s], sa[u][ks]);
    }
  }
  float m[2], l[2];
  if (nkw < KTILE) {                             // only the last wave's tile is ragged
#pragma unroll
    for (int u = 0; u < 2; ++u) mask_scores(sa[u], 0, nkw, h);
  }
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const float mt = score_max(sa[u], sl2);
    const f2 sl2v = {sl2, sl2}, nmt = {-mt, -mt};
    f2 rs2 = {0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int i = 0; i < 16; i += 2) {
        const f2 a = f2{sa[u][ks][i], sa[u][ks][i + 1]} * sl2v + nmt;
        const f2 p = {fexp2(a.x), fexp2(a.y)};
        sa[u][ks][i] = p.x;
        sa[u][ks][i + 1] = p.y;
        rs2 += p;
      }
    const float rs = rs2.x + rs2.y;
    m[u] = mt;
    l[u] = rs + xor_lane<32>(rs);
  }
  // this wave's (max, sum) per query into its K image (K is no longer read)
  float* st = reinterpret_cast<float*>(Ki);
  if (h == 0) {
#pragma unroll
    for (int u = 0; u < 2; ++u) { st[32 * u + r] = m[u]; st[64 + 32 * u + r] = l[u]; }
  }
  f32x16 acc[2][2];
#pragma unroll
  for (int u = 0; u < 2; ++u) acc[u][0] = acc[u][1] = zero16();
#pragma unroll
  for (int ks = 0; ks < 2; ++ks)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const frag8<E> v0 = frag_t<E>(Vi, 32 * ks, 0, s, lane);
      const frag8<E> v1 = frag_t<E>(Vi, 32 * ks, 32, s, lane);
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const frag8<E> pf = MF<E>::from_acc(sa[u][ks], s);
        acc[u][0] = MF<E>::mma(v0, pf, acc[u][0]);
        acc[u][1] = MF<E>::mma(v1, pf, acc[u][1]);
      }
    }
  __syncthreads();                               // every wave's (max, sum) is in LDS
  float mul[2], M[2], L[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    float mx = -INFINITY;
    for (int w = 0; w < nw; ++w) mx = fmaxf(mx, reinterpret_cast<const float*>(smem + w * SREG)[32 * u + r]);
    float sum = 0.f;
    for (int w = 0; w < nw; ++w) {
      const float* sw = reinterpret_cast<const float*>(smem + w * SREG);
      sum += sw[64 + 32 * u + r] * fexp2(sw[32 * u + r] - mx);
    }
    M[u] = mx;
    L[u] = sum;
    mul[u] = fexp2(m[u] - mx) / sum;             // this wave's share of the normalised output
  }
  __syncthreads();                               // the statistics are read: the regions take the outputs
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    put_tile(Ki, acc[u][0], 32 * u, 0, lane, mul[u]);
    put_tile(Ki, acc[u][1], 32 * u, 1, lane, mul[u]);
    const int qi = q0 + 32 * u + r;
    if (wave == 0 && h == 0 && lse && qi < N)
      lse[((long)b * heads + head) * N + qi] = (M[u] + __log2f(L[u])) * 0.69314718055994531f;
  }
  sum_store_queries(smem, nw, 64, o, b, head, N, q0, os);
}

// dQ: workgroup = 64 queries of one (b, head); wave w = key tile w; partial dQ summed in LDS
template <typename E>
__global__ __launch_bounds__(64 * SKT) void sra_dq_small(const E* __restrict__ q, const E* __restrict__ k,
                                                        const E* __restrict__ v, const E* __restrict__ o,
                                                        const E* __restrict__ dout, const float* __restrict__ lse,
                                                        float* __restrict__ Dws, E* __restrict__ dq, int N, int Nk,
                                                        int heads, long qs, long kvs, long os, long dos, long dqs,
                                                        float sl2, float scale) {
  __shared__ __attribute__((aligned(1024))) char smem[SKT * SREG];
  const int nw = blockDim.x >> 6;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int b = blockIdx.z, head = blockIdx.y, q0 = blockIdx.x * 64;
  char* Ki = smem + wave * SREG;
  char* Vi = Ki + KTILE * ROWB;
  const int t0 = wave * KTILE, nkw = min(KTILE, Nk - t0);
  stage_kv(k, v, b, head, Nk, kvs, t0, nkw, KTILE, Ki, Vi, 0, lane, 1);
  frag8<E> qf[2][4], df[2][4];
  float Dq[2], lse2[2];
#pragma unroll
  for (int u = 0; u < 2; ++u)
    sra_dq_row(q, o, dout, lse, Dws, b, head, heads, N, q0 + 32 * u + r, qs, os, dos, h, h == 0 && wave == 0,
               qf[u], df[u], Dq[u], lse2[u]);
  vm_wait<0>();
  f32x16 acc[2][2];
#pragma unroll
  for (int u = 0; u < 2; ++u) acc[u][0] = acc[u][1] = zero16();
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    frag8<E> kf[4], vf[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      kf[s] = frag_k<E>(Ki, 32 * ks, s, lane);
      vf[s] = frag_k<E>(Vi, 32 * ks, s, lane);
    }
    f32x16 ds[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      f32x16 sa = zero16(), dp = zero16();
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        sa = MF<E>::mma(kf[s], qf[u][s], sa);
        dp = MF<E>::mma(vf[s], df[u][s], dp);
      }
      dq_ds_tile(sa, dp, ds[u], sl2, lse2[u], Dq[u], 32 * ks, nkw, h, nkw < KTILE);
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const frag8<E> k0 = frag_t<E>(Ki, 32 * ks, 0, s, lane);
      const frag8<E> k1 = frag_t<E>(Ki, 32 * ks, 32, s, lane);
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const frag8<E> sf = MF<E>::from_acc(ds[u], s);
        acc[u][0] = MF<E>::mma(k0, sf, acc[u][0]);
        acc[u][1] = MF<E>::mma(k1, sf, acc[u][1]);
      }
    }
  }
  // own region: every read of it fed an MFMA whose result is in acc, so it is free
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    put_tile(Ki, acc[u][0], 32 * u, 0, lane, scale);
    put_tile(Ki, acc[u][1], 32 * u, 1, lane, scale);
  }
  sum_store_queries(smem, nw, 64, dq, b, head, N, q0, dqs);
}

// The same dQ with the two 32-query halves of a wave taken one after the other (their Q / dO
// fragments loaded per half) and the K and V fragments of a sub-tile live one at a time: under
// 168 VGPRs, so two 5-wave workgroups share a CU (sra_dq_small holds both halves: 223 VGPRs,
// one workgroup per CU -- stage 3 of B2 480 x 640 runs its 380 workgroups in 1.5 rounds).
// Same MFMA order per output element as sra_dq_small (bit-identical).  Default; CMX_SRA_DQ_SEQ=0
// restores sra_dq_small.  Standalone (scripts/bench_sra.py, Bt = 4): stage-3 backward 36.8 -> 34.5 us,
// stage 4 26.2 -> 25.0 us; the bench pairs are within noise (profiles/r05_dqseq_ab.txt).
template <typename E, int NU>
__global__ __launch_bounds__(64 * SKT, 2) void sra_dq_small_seq(const E* __restrict__ q, const E* __restrict__ k,
                                                               const E* __restrict__ v, const E* __restrict__ o,
                                                               const E* __restrict__ dout,
                                                               const float* __restrict__ lse, float* __restrict__ Dws,
                                                               E* __restrict__ dq, int N, int Nk, int heads, long qs,
                                                               long kvs, long os, long dos, long dqs, float sl2,
                                                               float scale) {
  __shared__ __attribute__((aligned(1024))) char smem[SKT * SREG];
  const int nw = blockDim.x >> 6;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int b = blockIdx.z, head = blockIdx.y, q0 = blockIdx.x * 32 * NU;
  char* Ki = smem + wave * SREG;
  char* Vi = Ki + KTILE * ROWB;
  const int t0 = wave * KTILE, nkw = min(KTILE, Nk - t0);
  stage_kv(k, v, b, head, Nk, kvs, t0, nkw, KTILE, Ki, Vi, 0, lane, 1);
  f32x16 acc[NU][2];
#pragma unroll
  for (int u = 0; u < NU; ++u) acc[u][0] = acc[u][1] = zero16();
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    frag8<E> qf[4], df[4];
    float Dq, lse2;
    sra_dq_row(q, o, dout, lse, Dws, b, head, heads, N, q0 + 32 * u + r, qs, os, dos, h, h == 0 && wave == 0,
               qf, df, Dq, lse2);
    if (u == 0) vm_wait<0>();                  // (the K / V images of this wave have landed)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      f32x16 sa = zero16(), dp = zero16();
#pragma unroll
      for (int s_ = 0; s_ < 4; ++s_) sa = MF<E>::mma(frag_k<E>(Ki, 32 * ks, s_, lane), qf[s_], sa);
#pragma unroll
      for (int s_ = 0; s_ < 4; ++s_) dp = MF<E>::mma(frag_k<E>(Vi, 32 * ks, s_, lane), df[s_], dp);
      dq_ds_tile(sa, dp, sa, sl2, lse2, Dq, 32 * ks, nkw, h, nkw < KTILE);   // dS over S, pair by pair
#pragma unroll
      for (int s_ = 0; s_ < 2; ++s_) {
        const frag8<E> sf = MF<E>::from_acc(sa, s_);
        acc[u][0] = MF<E>::mma(frag_t<E>(Ki, 32 * ks, 0, s_, lane), sf, acc[u][0]);
        acc[u][1] = MF<E>::mma(frag_t<E>(Ki, 32 * ks, 32, s_, lane), sf, acc[u][1]);
      }
    }
  }
  // own region: every read of it fed an MFMA whose result is in acc, so it is free
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    put_tile(Ki, acc[u][0], 32 * u, 0, lane, scale);
    put_tile(Ki, acc[u][1], 32 * u, 1, lane, scale);
  }
  sum_store_queries(smem, nw, 32 * NU, dq, b, head, N, q0, dqs);
}

// dK / dV: workgroup = 32 keys of one (b, head) on the lanes; wave w sweeps query tiles
// w, w + nw, ... (its own Q / dO images), and the waves' sums meet in LDS: every key's dK / dV
// is complete inside the workgroup (written directly, no slabs)
template <typename E>
__global__ __launch_bounds__(64 * SQW) void sra_dkv_small(const E* __restrict__ q, const E* __restrict__ k,
                                                         const E* __restrict__ v, const E* __restrict__ dout,
                                                         const float* __restrict__ lse, const float* __restrict__ Dws,
                                                         E* __restrict__ dk, E* __restrict__ dv, long dkvs, int N,
                                                         int Nk, int heads, long qs, long kvs, long dos, float sl2,
                                                         float scale) {
  __shared__ __attribute__((aligned(1024))) char smem[SQW * SDREG];
  const int nw = blockDim.x >> 6;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int head = blockIdx.y, b = blockIdx.z, k0 = blockIdx.x * 32;
  const long sbase = ((long)b * heads + head) * N;
  const i32x4 rq = make_rsrc(q + (long)b * N * qs + head * HD);
  const i32x4 rd = make_rsrc(dout + (long)b * N * dos + head * HD);
  const i32x4 rl = make_rsrc(lse + sbase);
  const i32x4 rD = make_rsrc(Dws + sbase);
  char* Qi = smem + wave * SDREG;
  char* Di = Qi + KTILE * ROWB;
  const float* ls = reinterpret_cast<const float*>(Qi + 2 * KTILE * ROWB);
  const float* Ds = ls + KTILE;
  const int key = k0 + r;
  frag8<E> kf[4], vf[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    if (key < Nk) {
      kf[s] = frag_bits<E>(*reinterpret_cast<const uint4*>(k + ((long)b * Nk + key) * kvs + head * HD + 16 * s + 8 * h));
      vf[s] = frag_bits<E>(*reinterpret_cast<const uint4*>(v + ((long)b * Nk + key) * kvs + head * HD + 16 * s + 8 * h));
    } else {
      kf[s] = vf[s] = zfrag<E>();
    }
  }
  f32x16 ak[2], av[2];
  ak[0] = ak[1] = av[0] = av[1] = zero16();
  const int nqt = (N + KTILE - 1) / KTILE;
  for (int qt0 = wave; qt0 < nqt; qt0 += nw) {
    const int q0 = qt0 * KTILE;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the previous tile's image reads are done
    // this tile's Q / dO rows (8 + 8 instructions) and lse / Dq (one each) into the wave's images
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int row = j * 8 + (lane >> 3), cc = (lane & 7) ^ swz(row), gq = q0 + row;
      dma16(rq, lds_addr(Qi + j * 1024), gq < N ? (int)(((long)gq * qs + cc * 8) * 2) : OOB);
      dma16(rd, lds_addr(Di + j * 1024), gq < N ? (int)(((long)gq * dos + cc * 8) * 2) : OOB);
    }
    dma4(rl, lds_addr(Qi + 2 * KTILE * ROWB), q0 + lane < N ? (q0 + lane) * 4 : OOB);
    dma4(rD, lds_addr(Qi + 2 * KTILE * ROWB + KTILE * 4), q0 + lane < N ? (q0 + lane) * 4 : OOB);
    vm_wait<0>();
#pragma unroll
    for (int qh = 0; qh < 2; ++qh) {
      const int qb = 32 * qh;
      f32x16 sa = zero16(), dp = zero16();
#pragma unroll
      for (int s = 0; s < 4; ++s) sa = MF<E>::mma(frag_k<E>(Qi, qb, s, lane), kf[s], sa);
#pragma unroll
      for (int s = 0; s < 4; ++s) dp = MF<E>::mma(frag_k<E>(Di, qb, s, lane), vf[s], dp);
      const bool tail = q0 + qb + 32 > N;
      const f2 sl2v = {sl2, sl2}, nlog2e = {-1.4426950408889634f, -1.4426950408889634f};
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const float4 l4 = *reinterpret_cast<const float4*>(ls + qb + 8 * g4 + 4 * h);
        const float4 d4 = *reinterpret_cast<const float4*>(Ds + qb + 8 * g4 + 4 * h);
#pragma unroll
        for (int e = 0; e < 4; e += 2) {
          const int i = 4 * g4 + e;
          const f2 lv = e == 0 ? f2{l4.x, l4.y} : f2{l4.z, l4.w};
          const f2 dv2 = e == 0 ? f2{d4.x, d4.y} : f2{d4.z, d4.w};
          const f2 a = f2{sa[i], sa[i + 1]} * sl2v + lv * nlog2e;
          f2 p = {fexp2(a.x), fexp2(a.y)};
          if (tail) {                            // uniform: only the ragged last query tile
            if (q0 + qb + accrow(i, h) >= N) p.x = 0.f;
            if (q0 + qb + accrow(i + 1, h) >= N) p.y = 0.f;
          }
          const f2 d = p * (f2{dp[i], dp[i + 1]} - dv2);
          sa[i] = p.x; sa[i + 1] = p.y;
          dp[i] = d.x; dp[i + 1] = d.y;
        }
      }
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const frag8<E> pf = MF<E>::from_acc(sa, s);
        const frag8<E> sf = MF<E>::from_acc(dp, s);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          av[t] = MF<E>::mma(frag_t<E>(Di, qb, 32 * t, s, lane), pf, av[t]);
          ak[t] = MF<E>::mma(frag_t<E>(Qi, qb, 32 * t, s, lane), sf, ak[t]);
        }
      }
    }
  }
  // the waves' partial sums meet in LDS: [key][d] dK tile then dV tile in each wave's region
  // (its images are dead: every read fed an MFMA whose result is in ak / av)
  put_tile(Qi, ak[0], 0, 0, lane, scale);
  put_tile(Qi, ak[1], 0, 1, lane, scale);
  put_tile(Qi + 32 * 256, av[0], 0, 0, lane, 1.f);
  put_tile(Qi + 32 * 256, av[1], 0, 1, lane, 1.f);
  __syncthreads();
  for (int it = threadIdx.x; it < 2 * 32 * 8; it += blockDim.x) {
    const int which = it >> 8, row = (it >> 3) & 31, dg = it & 7, kk = k0 + row;
    if (kk >= Nk) continue;
    E* out = (which ? dv : dk) + ((long)b * Nk + kk) * dkvs + head * HD + 8 * dg;
    sum_store8<E>(smem + which * 32 * 256, nw, SDREG, row, dg, 1.f, out);
  }
}

// CU count of the current device (pick_nw, sra_plan.h); 256 when it cannot be read
int sra_cus() {
  static const int n = [] {
    int dev = 0, c = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) !=
                                               hipSuccess)
      c = 0;
    return c > 0 ? c : 256;
  }();
  return n;
}

// the tile constants plan_sra counts with are the kernels'
static_assert(sraplan::HD == HD && sraplan::NKP_MAX == NKP_MAX && sraplan::NWAVE == NWAVE && sraplan::QT == QT,
              "sra_plan.h and sra_fast.hip disagree on a tile constant");

// knobs are read when a launch is planned (eager call or graph capture)
sraplan::SraKnobs sra_knobs() {
  static const sraplan::SraKnobs def;            // the defaults live in sra_plan.h
  static int& small_n = cmx_knob("SRA_SMALL_N", def.small_n);
  static int& small_fwd_n = cmx_knob("SRA_SMALL_FWD_N", def.small_fwd_n);
  static int& dq_seq = cmx_knob("SRA_DQ_SEQ", def.dq_seq);
  static int& qw = cmx_knob("SRA_QW", def.qw);
  static int& nw = cmx_knob("SRA_NW", def.nw);
  static int& dkv_direct = cmx_knob("SRA_DKV_DIRECT", def.dkv_direct);
  sraplan::SraKnobs k;
  k.small_n = small_n;
  k.small_fwd_n = small_fwd_n;
  k.dq_seq = dq_seq;
  k.qw = qw;
  k.nw = nw;
  k.dkv_direct = dkv_direct;
  return k;
}

// ---------------------------------------------------------------- launch dispatch
template <typename E> struct Elem { using type = E; };
template <int V> using Int = std::integral_constant<int, V>;

// f(Elem<bf16 or f16>): the plan said SRA_FAST or SRA_SMALL, so dtype is 1 (bf16) or 2 (fp16)
template <typename F>
void by_dtype(int dtype, F&& f) {
  if (dtype == 2) f(Elem<f16>{});
  else f(Elem<bf16>{});
}

// f(Int<QW>, Int<NW>) for the plan's (qw, nw): the six instantiations of sra_fwd_fast / sra_dq_fast
template <typename F>
void by_qw_nw(int qw, int nw, F&& f) {
  if (qw == 2 && nw == 4) f(Int<2>{}, Int<4>{});
  else if (qw == 2) f(Int<2>{}, Int<8>{});
  else if (nw == 10) f(Int<1>{}, Int<10>{});
  else if (nw == 8) f(Int<1>{}, Int<8>{});
  else if (nw == 4) f(Int<1>{}, Int<4>{});
  else f(Int<1>{}, Int<2>{});                    // pick_nw returns 2, 4, 8 or 10
}

}  // namespace

// the one launch decision of the SRA family (rules: sra_plan.h) under the live knobs and CU count;
// cmx_sra_attn_fwd / cmx_sra_attn_bwd launch from it and cmx_sra_plan reports it
sraplan::SraPlan sra_plan_now(int Bt, int N, int Nk, int heads, int D, int dtype, int aligned) {
  return sraplan::plan_sra(Bt, N, Nk, heads, D, dtype, aligned, sra_knobs(), sra_cus());
}

// fast dK / dV query chunks under the live knobs (workspace sizing)
int sra_dkv_fast_chunks(int Bt, int N, int Nk, int heads) {
  return sraplan::fast_dkv_chunks(Bt, N, Nk, heads, sra_knobs());
}

// The forward of an eligible problem (sra_plan.h: 16-bit storage, D = 64, 16-B aligned rows).
// Short sequences (Nk <= 320, one 64-key tile per wave, N <= CMX_SRA_SMALL_N, default 2048: stages
// 3 / 4 of B2 / B4) have their own kernels, but the forward takes its short-sequence kernel only up to
// CMX_SRA_SMALL_FWD_N queries (default 600: stage 4; stage 3's N = 1200 runs the general LDS-resident
// forward).  Measured standalone (profiles/r05_e_sra_standalone.txt, Bt = 4, Nk = 300): N = 1200 x 5
// heads 16.0 us small vs 11.9 us fast; N = 300 x 8 heads 9.0 vs 10.6 us.  Both forwards sit at the same
// error against fp64 at the B2 / B4 stage-3 / 4 shapes
// (tests/test_gpu_kernels.py::test_sra_fwd_kernel_choice); the round-5 config-4 trip
// (FRMs.3.channel_weights.mlp.0.bias ratio 18.4) was the parity test's ReLU-band cap, which now excludes
// exactly the rows whose ReLU decision flipped
void sra_lds_fwd(const SraArgs& a, const sraplan::SraPlan& plan) {
  by_dtype(a.dtype, [&](auto elem) {
    using E = typename decltype(elem)::type;
    const E *q = (const E*)a.q, *k = (const E*)a.k, *v = (const E*)a.v;
    if (plan.fwd == sraplan::SRA_SMALL) {
      hipLaunchKernelGGL(sra_fwd_small<E>, dim3(cdiv(a.N, 64), a.heads, a.Bt), dim3(64 * cdiv(a.Nk, KTILE)), 0,
                         a.stream, q, k, v, (E*)a.o, a.lse, a.N, a.Nk, a.heads, a.qs, a.kvs, a.os, a.sl2);
      return;
    }
    const int nkp = (a.Nk + KTILE - 1) / KTILE * KTILE;
    by_qw_nw(plan.qw, plan.nw, [&](auto qw, auto nw) {
      constexpr int QW = decltype(qw)::value, NW = decltype(nw)::value;
      hipLaunchKernelGGL((sra_fwd_fast<E, QW, NW>), dim3(cdiv(a.N, 32 * NW * QW), a.heads, a.Bt), dim3(64 * NW), 0,
                         a.stream, q, k, v, (E*)a.o, a.lse, a.N, a.Nk, nkp, a.heads, a.qs, a.kvs, a.os, a.sl2);
    });
  });
}

// The backward of an eligible problem: dQ (which also writes Dq to a.Dws), then dK / dV.  Fast: the
// dK / dV kernel writes plan.dkv_chunks partial slabs (layout of sra_attention.hip's general path, folded
// by the caller), or with one chunk the gradients themselves
void sra_lds_bwd(const SraArgs& a, const sraplan::SraPlan& plan) {
  by_dtype(a.dtype, [&](auto elem) {
    using E = typename decltype(elem)::type;
    const E *q = (const E*)a.q, *k = (const E*)a.k, *v = (const E*)a.v, *o = (const E*)a.o, *dout = (const E*)a.dout;
    if (plan.bwd == sraplan::SRA_SMALL) {
      const dim3 grid(cdiv(a.N, 64), a.heads, a.Bt), block(64 * cdiv(a.Nk, KTILE));
      // plan.dq_seq (CMX_SRA_DQ_SEQ, default 1): sra_dq_small_seq (0: sra_dq_small)
      if (plan.dq_seq)
        hipLaunchKernelGGL((sra_dq_small_seq<E, 2>), grid, block, 0, a.stream, q, k, v, o, dout, a.lse, a.Dws,
                           (E*)a.dq, a.N, a.Nk, a.heads, a.qs, a.kvs, a.os, a.dos, a.dqs, a.sl2, a.scale);
      else
        hipLaunchKernelGGL(sra_dq_small<E>, grid, block, 0, a.stream, q, k, v, o, dout, a.lse, a.Dws, (E*)a.dq, a.N,
                           a.Nk, a.heads, a.qs, a.kvs, a.os, a.dos, a.dqs, a.sl2, a.scale);
      const int nqt = cdiv(a.N, KTILE);
      hipLaunchKernelGGL(sra_dkv_small<E>, dim3(cdiv(a.Nk, 32), a.heads, a.Bt), dim3(64 * (nqt < SQW ? nqt : SQW)),
                         0, a.stream, q, k, v, dout, a.lse, a.Dws, (E*)a.dk, (E*)a.dv, a.dkvs, a.N, a.Nk, a.heads,
                         a.qs, a.kvs, a.dos, a.sl2, a.scale);
      return;
    }
    const int nkp = (a.Nk + KTILE - 1) / KTILE * KTILE;
    by_qw_nw(plan.qw, plan.nw, [&](auto qw, auto nw) {
      constexpr int QW = decltype(qw)::value, NW = decltype(nw)::value;
      hipLaunchKernelGGL((sra_dq_fast<E, QW, NW>), dim3(cdiv(a.N, 32 * NW * QW), a.heads, a.Bt), dim3(64 * NW), 0,
                         a.stream, q, k, v, o, dout, a.lse, a.Dws, (E*)a.dq, a.N, a.Nk, nkp, a.heads, a.qs, a.kvs,
                         a.os, a.dos, a.dqs, a.sl2, a.scale);
    });
    const int nchunk = plan.dkv_chunks;
    const int nkw = ((a.Nk < NKP_MAX ? a.Nk : NKP_MAX) + 31) / 32 * 32;   // one 32-key sub-tile per wave
    const int nkc = (a.Nk + NKP_MAX - 1) / NKP_MAX;                         // key chunks (Nk > NKP_MAX)
    int qc = (a.N + nchunk - 1) / nchunk;
    qc = (qc + QT - 1) / QT * QT;
    hipLaunchKernelGGL(sra_dkv_fast<E>, dim3(nchunk * nkc, a.heads, a.Bt), dim3(2 * nkw), 0, a.stream, q, k, v, dout,
                       a.lse, a.Dws, a.ws_dk, a.ws_dv, (E*)a.dk, (E*)a.dv, a.dkvs, a.Bt, a.N, a.Nk, a.heads, a.qs,
                       a.kvs, a.dos, qc, nchunk, a.sl2, a.scale);
  });
}
