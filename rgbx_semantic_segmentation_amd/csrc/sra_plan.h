// sra_plan.h -- the whole launch policy of the SRA attention family as plain host arithmetic:
// which forward and backward kernels a problem gets, the fast kernels' <QW, NW> instantiation,
// the dK / dV query chunks and the short-sequence dQ form.  No HIP in here and no state: the
// knobs and the CU count are arguments.  cmx_sra_attn_fwd / cmx_sra_attn_bwd launch from the
// SraPlan that sra_plan_now (sra_fast.hip) fills from the live knobs, and cmx_sra_plan returns
// the same struct to the tests: there is no second copy of these rules.
//
// Rule order of plan_sra:
//   1. eligibility  the LDS-resident kernels (sra_fast.hip) take 16-bit storage, D = 64 and 16-B
//                   aligned rows (`aligned` bit 0: q, k, v, o, dO, dq and their strides; bit 1:
//                   dK / dV); everything else runs the general kernels of sra_attention.hip
//   2. small        Nk <= 320 and N <= SRA_SMALL_N: the short-sequence backward (it also needs
//                   bit 1); with N <= SRA_SMALL_FWD_N as well: the short-sequence forward
//   3. fast         any other eligible problem; <QW, NW> from pick_qw / pick_nw
//   4. dK / dV      fast: fast_dkv_chunks query chunks (1 = written directly, no slabs, no reduce
//                   launch); general: general_dkv_chunks; small: one pass, written directly
#pragma once

namespace sraplan {

constexpr int HD = 64;          // head dim of the LDS-resident kernels
constexpr int NKP_MAX = 320;    // keys held in LDS
constexpr int NWAVE = 8;        // default waves per fast workgroup
constexpr int QT = 64;          // queries per fast dK / dV tile
constexpr int GEN_BK = 128;     // keys per general dK / dV workgroup
constexpr int GEN_KT = 32;      // queries per general LDS tile

inline long cdiv(long a, long b) { return (a + b - 1) / b; }

// every SRA launch-policy knob (CMX_<NAME> in the environment, cmx_tune in-process) at its default
struct SraKnobs {
  int small_n = 2048;      // SRA_SMALL_N: the largest N of the short-sequence backward
  int small_fwd_n = 600;   // SRA_SMALL_FWD_N: the largest N of the short-sequence forward
  int dq_seq = 1;          // SRA_DQ_SEQ: sra_dq_small_seq (0: sra_dq_small)
  int qw = 0;              // SRA_QW: 1 / 2 query sub-tiles per wave, 0 = auto
  int nw = 0;              // SRA_NW: 2 / 4 / 8 / 10 waves per workgroup, 0 = auto
  int dkv_direct = 0;      // SRA_DKV_DIRECT: the largest N whose fast dK / dV is written directly
};

enum SraPath { SRA_GENERAL = 0, SRA_FAST = 1, SRA_SMALL = 2 };

struct SraPlan {
  int fwd, bwd;            // SraPath of the forward / of the backward (dQ and dK / dV together)
  int qw, nw;              // <QW, NW> of sra_fwd_fast / sra_dq_fast (0 when neither is fast)
  int dkv_chunks;          // query chunks of the dK / dV kernel (slabs the reducer folds)
  int dkv_direct;          // dK / dV stored by the dK / dV kernel itself: no slabs, no reduce launch
  int dq_seq;              // backward small: sra_dq_small_seq (1) or sra_dq_small (0)
  int cus;                 // the CU count the rules used
};
constexpr int SRA_PLAN_INTS = sizeof(SraPlan) / sizeof(int);

// query sub-tiles per wave: 2 once that still leaves 512 workgroups
inline int pick_qw(int N, int heads, int Bt, const SraKnobs& kn) {
  if (kn.qw == 1 || kn.qw == 2) return kn.qw;
  const long wg2 = cdiv(N, 64 * NWAVE) * heads * Bt;   // workgroups at 2 sub-tiles per wave
  return wg2 >= 512 ? 2 : 1;
}

// waves per workgroup: 8 (two per SIMD share one K/V image) unless that leaves fewer than
// 128 workgroups (stage 3: 100, stage 4: 64 at B2 480x640), where 2-wave workgroups spread
// the work over 2.5-4x more CUs (measured: dQ 17.7 -> 14.8 us at stages 3 and 4; 4-wave
// workgroups at stage 2 (152 -> 304) were slower, 13.8 -> 16.4 us forward).  Every workgroup
// stages the (b, head)'s K / V (L2-resident after the first): only L2 -> LDS traffic.
// 10 waves when the 8-wave grid overflows one workgroup per CU and the 10-wave grid does not
// (stage 1 of B2 480 x 640: 300 -> 240 workgroups; measured fwd 19.6 -> 15.9 us, bwd 69.2 ->
// 61.6 us; the 44 CUs that ran a second 8-wave workgroup set the launch time.  At stage 2 the
// 8-wave grid already fits, and 10 waves were slower: 11.7 -> 14.2 us forward)
inline int pick_nw(int N, int heads, int Bt, int qw, const SraKnobs& kn, int cus) {
  const int force = kn.nw;
  if (force == 2 || force == 4 || force == 8) return qw == 2 && force == 2 ? 4 : force;
  if (force == 10 && qw == 1) return 10;
  if (qw == 1 && cdiv(N, 32 * NWAVE) * heads * Bt > cus && cdiv(N, 320) * heads * Bt <= cus) return 10;
  if (qw == 2 || cdiv(N, 32 * NWAVE) * heads * Bt >= 128) return NWAVE;
  return 2;
}

// fast dK / dV: query chunks per (image, head, 320-key chunk), ~one workgroup per CU over the
// whole grid (the SRA layers have one key chunk; IFFM's full cross attention has Nk / 320 of
// them, which already fill the chip, and every extra query chunk is another Nk x D slab to
// reduce).  Short query sequences (N <= SRA_DKV_DIRECT): one chunk, the gradients written
// directly (no fp32 slabs, no reduce launch)
inline int fast_dkv_chunks(int Bt, int N, int Nk, int heads, const SraKnobs& kn) {
  const long base = (long)Bt * heads * cdiv(Nk, NKP_MAX);
  if (N <= kn.dkv_direct) return 1;
  long nc = (256 + base - 1) / base;
  const long maxc = cdiv(N, QT);
  if (nc > maxc) nc = maxc;
  if (nc > 64) nc = 64;
  return (int)(nc < 1 ? 1 : nc);
}

// general dK / dV: query chunks per (image, head, 128-key block), ~512 workgroups
inline int general_dkv_chunks(int Bt, int N, int Nk, int heads) {
  const long base = (long)Bt * heads * cdiv(Nk, GEN_BK);
  long nc = (512 + base - 1) / base;
  const long maxc = cdiv(N, GEN_KT);
  if (nc > maxc) nc = maxc;
  if (nc < 1) nc = 1;
  return (int)nc;
}

// dtype 0 fp32 / 1 bf16 / 2 fp16; aligned: bit 0 = q, k, v, o (backward: dO, dq too) start on
// 16 B and their row strides are multiples of 8 elements, bit 1 = the same for dK / dV
inline SraPlan plan_sra(int Bt, int N, int Nk, int heads, int D, int dtype, int aligned, const SraKnobs& kn,
                        int cus) {
  SraPlan p = {};
  p.cus = cus;
  const bool lds = (dtype == 1 || dtype == 2) && D == HD && Nk > 0 && (aligned & 1);
  const bool small = lds && Nk <= NKP_MAX && N <= kn.small_n;
  p.fwd = small && N <= kn.small_fwd_n ? SRA_SMALL : lds ? SRA_FAST : SRA_GENERAL;
  p.bwd = small && (aligned & 2) ? SRA_SMALL : lds ? SRA_FAST : SRA_GENERAL;
  if (p.fwd == SRA_FAST || p.bwd == SRA_FAST) {
    p.qw = pick_qw(N, heads, Bt, kn);
    p.nw = pick_nw(N, heads, Bt, p.qw, kn, cus);
  }
  if (p.bwd == SRA_SMALL) {
    p.dkv_chunks = 1;
    p.dkv_direct = 1;
    p.dq_seq = kn.dq_seq != 0;
  } else if (p.bwd == SRA_FAST) {
    p.dkv_chunks = fast_dkv_chunks(Bt, N, Nk, heads, kn);
    p.dkv_direct = p.dkv_chunks == 1;
  } else {
    p.dkv_chunks = general_dkv_chunks(Bt, N, Nk, heads);
  }
  return p;
}

}  // namespace sraplan
