// sra_args.h -- what the two SRA translation units (sra_attention.hip: the C-ABI entry points and the
// general kernels; sra_fast.hip: the LDS-resident kernels) share on the host: the problem as one struct
// and the entry points of sra_fast.hip.  (sra_plan.h stays HIP-free; this header needs hipStream_t.)
#pragma once
#include "cmx_common.h"
#include "sra_plan.h"

// One attention problem as cmx_sra_attn_fwd / cmx_sra_attn_bwd receive it (layout: sra_attention.hip).
// The forward fills q, k, v, o, lse; the backward all of it (o and lse are then inputs).
struct SraArgs {
  const void *q, *k, *v;
  void* o;
  const void* dout;
  float *lse, *Dws;              // Dws (Bt, heads, N): Dq = rowsum(dO . O), written by dQ, read by dK / dV
  void *dq, *dk, *dv;
  float *ws_dk, *ws_dv;          // fp32 slabs of plan.dkv_chunks partial dK / dV (unused when dkv_direct)
  int Bt, N, Nk, heads, D;
  long qs, kvs, os, dos, dqs, dkvs;   // row strides in elements
  float sl2, scale;              // scale * log2(e), scale
  int dtype;
  hipStream_t stream;
};

// sra_fast.hip.  sra_plan_now is the launch decision (sra_plan.h) under the live knobs and CU count;
// sra_lds_fwd / sra_lds_bwd launch the fast or the short-sequence kernels the plan names (never called
// with SRA_GENERAL).  After sra_lds_bwd the caller folds the slabs unless plan.dkv_direct.
sraplan::SraPlan sra_plan_now(int Bt, int N, int Nk, int heads, int D, int dtype, int aligned);
int sra_dkv_fast_chunks(int Bt, int N, int Nk, int heads);
void sra_lds_fwd(const SraArgs& a, const sraplan::SraPlan& plan);
void sra_lds_bwd(const SraArgs& a, const sraplan::SraPlan& plan);
