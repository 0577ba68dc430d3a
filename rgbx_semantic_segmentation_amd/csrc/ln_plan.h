// ln_plan.h -- the whole launch policy of the LayerNorm kernels (layernorm.hip) as plain host
// arithmetic: the <TPR, NCH, RPT> instantiation of ln_fwd_kernel / ln_bwd_kernel a problem gets,
// its grid, the backward's block count per group and its workspace.  No HIP in here and no
// state.  ln_fwd_launch, ln_bwd_launch and cmx_layernorm_bwd_workspace all read the LnPlan below,
// and tests/host/ln_plan_dump.cpp prints the same struct: there is no second copy of these rules.
//
//   V     elements per 16-byte vector: 4 (fp32) or 8 (bf16 / fp16); C is a multiple of V, <= 1024
//   tpr   lanes per row: the row's C / V chunks rounded up to a power of two, 4 .. 64
//   nch   chunks per lane: 1, 2 or 4.  Three (fp32, 512 < C <= 768) runs the NCH = 4 kernels,
//         whose `ch < nchunk` masks already leave a lane's chunks past the row alone
//   rpt   rows per thread with their loads in flight together; more than one only for narrow
//         rows (nch = 1, tpr <= 16): forward 4 when that still leaves 256 blocks (one per CU),
//         backward 2 when a thread walks more than one row
//   nb    backward: blocks per group, at most LN_BWD_MAX_BLOCKS (~2 rows per thread at stage 1);
//         each leaves one [dgamma C | dbeta C] fp32 partial in the workspace (G, nb, 2C)
#pragma once

#include <stddef.h>

namespace lnplan {

constexpr int BLOCK = 256;                 // threads per block of both kernels
constexpr int LN_MAX_C = 1024;
constexpr int LN_BWD_MAX_BLOCKS = 512;

struct LnPlan {
  int tpr, nch, rpt;
  int rpb;                 // rows per block and step: BLOCK / tpr
  unsigned grid_x, grid_y;
  int nb;                  // backward: blocks per group (= grid_x); forward: 0
  size_t ws_bytes;         // backward: G * nb * 2C floats; forward: 0
};

inline int vec_width(int dtype) { return dtype == 0 ? 4 : 8; }

inline int ln_tpr(int chunks) {
  int t = 1;
  while (t < chunks && t < 64) t <<= 1;
  return t < 4 ? 4 : t;
}

inline int ln_nch(int chunks, int tpr) {
  const int n = (chunks + tpr - 1) / tpr;
  return n == 3 ? 4 : n;
}

inline int ln_bwd_blocks(long R, int rpb) {
  const long nb = (R + rpb - 1) / rpb;
  return (int)(nb < LN_BWD_MAX_BLOCKS ? nb : LN_BWD_MAX_BLOCKS);
}

inline LnPlan plan_ln_fwd(long R, int G, int C, int V) {
  LnPlan p = {};
  p.tpr = ln_tpr(C / V);
  p.nch = ln_nch(C / V, p.tpr);
  p.rpb = BLOCK / p.tpr;
  p.rpt = (p.nch == 1 && p.tpr <= 16 && R * G / (p.rpb * 4) >= 256) ? 4 : 1;
  const long per_block = (long)p.rpb * p.rpt;
  p.grid_x = (unsigned)((R + per_block - 1) / per_block);
  p.grid_y = (unsigned)G;
  return p;
}

inline LnPlan plan_ln_bwd(long R, int G, int C, int V) {
  LnPlan p = {};
  p.tpr = ln_tpr(C / V);
  p.nch = ln_nch(C / V, p.tpr);
  p.rpb = BLOCK / p.tpr;
  p.nb = ln_bwd_blocks(R, p.rpb);
  p.rpt = (p.nch == 1 && p.tpr <= 16 && R > (long)p.nb * p.rpb) ? 2 : 1;
  p.grid_x = (unsigned)p.nb;
  p.grid_y = (unsigned)G;
  p.ws_bytes = (size_t)G * p.nb * 2 * C * sizeof(float);
  return p;
}

}  // namespace lnplan
