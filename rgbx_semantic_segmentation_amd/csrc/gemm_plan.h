// gemm_plan.h -- the whole launch policy of the MFMA GEMM family as plain host arithmetic: which
// kernel, which tile, how many waves, how many splits and which grid a problem gets.  No HIP in
// here (it compiles with any C++17 host compiler; tests/test_gemm_plan.py pins every rule against
// tests/golden/gemm_plans.tsv), and no state: the knobs and the CU count are arguments.
//
// Rule order of plan_gemm (first match wins inside a step; the steps run in this order):
//   1. split      a requested splitk > 0 is taken as is; otherwise the 16-bit path asks
//                 auto_split (1a-1d) and the generic path generic_split (1e)
//      1a. tiles of plan_tiles (step 3) >= 128 (200 at GEMM_TILES=0), or fewer than 8 k-tiles: 1
//      1b. GEMM_SPLITKW: 64 x 64 tiles, no bias-gradient column, <= 32 k-tiles: 1 (k-group waves, 5)
//      1c. ceil(256 / tiles) splits, each >= 4 k-tiles, at most 128
//      1d. no empty splits (split_k)
//      1e. generic: 1024 / tiles splits, each >= 8 k-tiles of 32, at most 64
//   2. path       generic unless `fast`: tile = 64 for a side <= 64, else 128 (the bias-gradient
//                 column counts as a column here); grid (tiles, G, nsplit); then step 7
//   3. tile       plan_tiles: 128 per side > 64; GEMM_T128: under 400 such tiles -> 64 x 64;
//                 GEMM_SMALLK: K <= 256 or a narrow output (nb <= 64) -> 64 x 64;
//                 a LayerNorm epilogue: 64 rows x the whole row (64 / 128, or the scatter's C)
//   4. MID        GEMM_MID: 64 x 64 tiles overflowing 5 blocks per CU by <= 50 % -> 64 x 128
//   5. stream     GEMM_STREAM: >= 1024 64 x 64 tiles with K <= 128 -> the resident streaming grid
//                 (GEMM_STREAM_BPC blocks per CU); otherwise one block per tile and split with
//                 NS / KW from tile_waves: GEMM_KW k-group waves for small 64 x 64 grids, a 4-slot
//                 ring up to 256 blocks, else 2 slots
//   6. (steps 4 and 5's stream rule are skipped for `tile_only` problems: the implicit conv and
//      the planning of a multi launch)
//   7. reducer    nsplit > 1: ZL 16 / 4 / 1 z-lanes for >= 32 / >= 8 / fewer slabs
// plan_multi and plan_grouped are the same pieces for a combined and a grouped launch.
#pragma once
#include <stdint.h>

#ifndef CMX_STREAM_LB
#define CMX_STREAM_LB 4                          // resident blocks per CU of the streaming kernel
#endif

namespace gemmplan {

constexpr int FAST_BK = 64, GENERIC_BK = 32;    // k per tile of the 16-bit / the generic kernel

inline long cdiv(long a, long b) { return (a + b - 1) / b; }

// every launch-policy knob (CMX_<NAME> in the environment, cmx_tune in-process) at its default
struct GemmKnobs {
  int tiles = 1;                   // GEMM_TILES
  int smallk = 256;                // GEMM_SMALLK
  int t128 = 400;                  // GEMM_T128
  int splitkw = 1;                 // GEMM_SPLITKW
  int kw = 2;                      // GEMM_KW
  int mid = 50;                    // GEMM_MID
  int stream = 1024;               // GEMM_STREAM
  int stream_k = 128;              // GEMM_STREAM_K
  int stream_bpc = CMX_STREAM_LB;  // GEMM_STREAM_BPC
  int grouped_kt = 48;             // GROUPED_KT
};

// everything the decision depends on
struct GemmShape {
  int G = 1, M = 0, N = 0, K = 0;
  int transA = 0, transB = 0, ones_col = 0, dtype = 1;
  int fast = 0;        // operands eligible for the LDS-DMA path (fast_ok and 16-B head strides)
  int splitk = 0;      // requested split, 0 = auto
  int a2 = 0;          // second A segment
  int row_ln = 0;      // LayerNorm of the output rows in the epilogue
  int ln_bwd = 0;      // LayerNorm backward in the epilogue
  int scC = 0;         // patch-scatter epilogue: its channel count (0 = no scatter)
  int nup = 0;         // upsample-add sources
  int gh = 1;          // inner count of a two-level batch
  int tile_only = 0;   // implicit conv / multi planning: no MID and no stream rule
};

enum GemmPath { PATH_GENERIC = 0, PATH_TILE = 1, PATH_STREAM = 2 };

struct GemmLaunch {
  int path, bm, bn, ns, kw;                    // kernel: tile, LDS ring slots, k-group waves
  int nsplit, kt_per_split, tiles_m, tiles_n;
  unsigned grid_x, grid_y, grid_z, block;
  int red_zl;                                  // split-K reducer (nsplit > 1): z-lanes and grid
  unsigned red_grid_x, red_grid_y;
};

inline int tile_dim(int n) { return n <= 64 ? 64 : 128; }

// k-tiles per split for `parts` requested splits, and the split count without empty splits
struct KSplit { int kt, n; };
inline KSplit split_k(int nk, int parts) {
  const int kt = (int)cdiv(nk, parts);
  return {kt, (int)cdiv(nk, kt)};
}

// Tile policy of the 16-bit path (GEMM_TILES=0 restores the 128-wide-first policy, for A/B
// measurements).  Policy 1: when 128-wide tiles leave the chip under-filled (< 400 tiles),
// take 64 x 64 tiles -- 4x the tiles, a lighter per-block k-loop and no split-K combine --
// and split K only when even those leave it under-filled.
inline void plan_tiles(int G, int M, int nb, int K, const GemmKnobs& k, int* bm, int* bn) {
  *bm = tile_dim(M);
  *bn = tile_dim(nb);
  // (GEMM_T128, default 400: the stage-3 MLP GEMMs, 380 128-wide tiles, run 64 x 64;
  // measured +0.6 % per step over 240 in interleaved A/B)
  if (k.tiles == 1 && cdiv(M, *bm) * cdiv(nb, *bn) * G < k.t128) *bm = *bn = 64;
  // Small-K policy (GEMM_SMALLK=k, default 256): problems with K <= k take 64 x 64 tiles
  // whatever their tile count -- a block of one to four k-tiles is a latency chain (DMA, MFMA,
  // epilogue), and the 128 x 128 tile's 67 KB epilogue image allows only two such chains per CU
  // where 64 x 64 blocks (32 KB) run four or more.  Measured on the B2 step's GEMM census
  // (profiles/r02_r_gemm_census.txt): the stage-1/2 MLP and decoder-input GEMMs
  // (M 38400 / 9600, K 64-256) gain 10-25 % each, 2558 -> 2485 us per step at k = 640; the one
  // 512 x 512 decoder GEMM (K 512) is the shape that keeps 128-wide tiles faster, hence 256.
  // A narrow output (N <= 64, K 512: the decoder's class / c1 products) also takes 64 x 64.
  if (K <= k.smallk || (nb <= 64 && k.smallk > 0)) *bm = *bn = 64;
}

// split factor for the 16-bit path: one block per CU when the output has few tiles (each split
// keeps >= 4 k-tiles of 64; the slabs cost 8 B of HBM traffic per output element and split)
inline int auto_split(int G, int M, int N, int K, int ones_col, const GemmKnobs& k) {
  const int nb = ones_col ? N - 1 : N;
  int bm, bn;
  plan_tiles(G, M, nb, K, k, &bm, &bn);
  const long tiles = cdiv(M, bm) * cdiv(nb, bn) * G;
  const int nk = (int)cdiv(K, FAST_BK);
  if (tiles >= (k.tiles == 1 ? 128 : 200) || nk < 8) return 1;
  // an under-filled 64 x 64 problem without a bias-gradient column runs as k-group blocks
  // (tile_waves, KW waves per tile) instead of split-K slabs + a reducer launch: measured
  // +1.2 % per step (interleaved A/B, 246.7 / 247.1 -> 249.5 / 250.5 img/s; GEMM_SPLITKW=0
  // restores split-K)
  // (short k-loops only: a k-group block walks nk / 2 ring slots serially, and the FFM context
  // products -- 64 x 64 over 19200 tokens, nk = 300 -- keep split-K: 10.8 vs 33 us)
  if (k.splitkw && bm == 64 && bn == 64 && !ones_col && nk <= 32) return 1;
  long s = cdiv(256, tiles);
  if (s > nk / 4) s = nk / 4;
  if (s > 128) s = 128;
  return split_k(nk, (int)s).n;
}

// split factor for the generic path: BK = 32, aim for ~1024 blocks with >= 8 k-tiles per split.
// (Quirk, kept: the bias-gradient column counts as an output column here, `ones_col ? N : N`
// in the code this came from, while the 16-bit path leaves it out.)
inline int generic_split(int G, int M, int N, int K) {
  const long tiles = cdiv(M, tile_dim(M)) * cdiv(N, tile_dim(N)) * G;
  const int nk = (int)cdiv(K, GENERIC_BK);
  long s = 1024 / tiles;
  if (s > nk / 8) s = nk / 8;
  if (s > 64) s = 64;
  return s < 1 ? 1 : (int)s;
}

// the library's split for a problem whose workspace the caller sizes before the launch
// (cmx_gemm_splitk).  (Quirk, kept: a 16-bit problem gets the 64-wide-k auto_split answer before
// anyone knows whether its operands are eligible for the 16-bit path; the generic kernel then
// runs that split over its 32-wide k-tiles.)
inline int default_split(int G, int M, int N, int K, int ones_col, int dtype, const GemmKnobs& k) {
  if (G <= 0 || M <= 0 || N <= 0 || K <= 0) return 1;
  return dtype == 1 || dtype == 2 ? auto_split(G, M, N, K, ones_col, k) : generic_split(G, M, N, K);
}

// split for a problem inside a grouped launch: the launch is filled by many problems, so a
// split only bounds the k-loop of one block.
// <= 48 k-tiles of 64 tokens per block (GROUPED_KT): measured against 16 / 24 / 32 / 64
// on the B2 step (interleaved A/B: 32 -> 48 is +1.5 %, 64 no better; fewer slabs to reduce)
inline int grouped_split(int K, const GemmKnobs& k) {
  const int nk = (int)cdiv(K, FAST_BK);
  long s = cdiv(nk, k.grouped_kt);
  if (s > 64) s = 64;
  return split_k(nk, (int)s).n;
}

// LDS ring slots and k-group waves of a one-block-per-tile launch of `blocks` blocks.
// k-group blocks for 64 x 64 tiles without split-K or bias column (GEMM_KW = the largest
// group count allowed, default 2; 1 = off).  Measured (scripts/gemm_sweep.py, G2 M600 N512):
// K 2048 20.1 -> 11.9 us, K 512 7.5 -> 5.8 us at KW = 2; grids above 512 blocks and one-slot
// problems are slower with it (M9600 N128 K512: 9.7 -> 10.4 us), so they keep 4 waves.
inline void tile_waves(GemmLaunch& L, long blocks, int nk64, int kw_max, bool kgroups_ok) {
  L.kw = 1;
  if (kgroups_ok && kw_max >= 2 && blocks <= 512 && nk64 >= 4) L.kw = kw_max >= 4 && blocks <= 256 && nk64 >= 16 ? 4 : 2;
  L.ns = L.kw == 4 || blocks > 256 ? 2 : 4;
  if (L.kw > 1) L.kt_per_split = split_k(nk64, L.kw).kt;
  L.grid_x = (unsigned)blocks; L.grid_y = L.grid_z = 1;
  L.block = 256u * L.kw;
}

inline GemmLaunch plan_gemm(const GemmShape& p, const GemmKnobs& k, int num_cu) {
  GemmLaunch L{};
  const int nb = p.ones_col ? p.N - 1 : p.N;
  const int split = p.splitk > 0 ? p.splitk
                    : p.fast     ? auto_split(p.G, p.M, p.N, p.K, p.ones_col, k)
                                 : generic_split(p.G, p.M, p.N, p.K);
  const int nk = (int)cdiv(p.K, p.fast ? FAST_BK : GENERIC_BK);
  const KSplit ks = split_k(nk, split);
  L.kt_per_split = ks.kt; L.nsplit = ks.n;
  L.kw = 1; L.block = 256;
  if (!p.fast) {
    // tile shape: the output's narrow side gets 64 (stage-1 C = 64 outputs, 64-row wgrads)
    L.path = PATH_GENERIC;
    L.bm = tile_dim(p.M); L.bn = tile_dim(p.N);
    L.tiles_m = (int)cdiv(p.M, L.bm); L.tiles_n = (int)cdiv(p.N, L.bn);
    L.grid_x = (unsigned)(L.tiles_m * L.tiles_n); L.grid_y = (unsigned)p.G; L.grid_z = (unsigned)L.nsplit;
  } else {
    plan_tiles(p.G, p.M, nb, p.K, k, &L.bm, &L.bn);
    if (p.row_ln || p.ln_bwd) L.bm = 64, L.bn = p.N <= 64 ? 64 : 128;   // one tile spans the row
    if (p.ln_bwd && p.scC) L.bn = p.scC;                                 // (one tap's C channels)
    const bool plain64 = L.bm == 64 && L.bn == 64 && L.nsplit == 1 && !p.tile_only && !p.ln_bwd && !p.scC && !p.nup;
    // 64 x 64 tiles that overflow one round of resident blocks by less than GEMM_MID percent
    // (5 per CU) take 64 x 128 tiles instead: one round of blocks twice as long, not a second
    // partial round (0 = off; default 50: GEMM census 1380 -> 1361 us, stage-3 fc1 14.3 -> 13.0 us)
    if (k.mid > 0 && plain64 && !p.row_ln && nb >= 128) {
      const long t64 = cdiv(p.M, 64) * cdiv(nb, 64) * p.G, slots = 5L * num_cu;
      if (t64 > slots && t64 * 100 <= slots * (100 + k.mid)) L.bn = 128;
    }
    L.tiles_m = (int)cdiv(p.M, L.bm); L.tiles_n = (int)cdiv(nb, L.bn);
    const long tiles = (long)L.tiles_m * L.tiles_n * p.G;
    // tall 64 x 64 problems of at least GEMM_STREAM tiles (0 = off) and K <= GEMM_STREAM_K:
    // the resident streaming grid (gemm_stream_kernel) instead of one block per tile
    if (k.stream > 0 && tiles >= k.stream && p.K <= k.stream_k && plain64 && L.bn == 64 && !p.transA && !p.a2 &&
        !p.ones_col && p.gh == 1 && (!p.row_ln || p.N <= 64)) {
      L.path = PATH_STREAM;
      const int bpc = k.stream_bpc > 0 && k.stream_bpc <= CMX_STREAM_LB ? k.stream_bpc : CMX_STREAM_LB;
      long grid = (long)bpc * num_cu;               // resident blocks per CU (VGPR-bound)
      if (grid > tiles) grid = tiles;
      L.grid_x = (unsigned)((grid + 7) / 8 * 8); L.grid_y = L.grid_z = 1;
    } else {
      L.path = PATH_TILE;
      tile_waves(L, tiles * L.nsplit, (int)cdiv(p.K, FAST_BK), k.kw,
                 L.bm == 64 && L.bn == 64 && L.nsplit == 1 && !p.ones_col);
    }
  }
  if (L.nsplit > 1) {
    const long work = (long)p.M * cdiv(nb, 8) + (p.ones_col ? p.M : 0);
    L.red_zl = L.nsplit >= 32 ? 16 : L.nsplit >= 8 ? 4 : 1;
    L.red_grid_x = (unsigned)cdiv(work, 256 / L.red_zl); L.red_grid_y = (unsigned)p.G;
  }
  return L;
}

// blocks of a problem planned for a multi launch (plan_gemm of a `tile_only` shape), 0 = not
// eligible: the 16-bit path on 64 x 64 tiles, no split-K, no bias-gradient column / upsample /
// scatter / two-level batch
inline int multi_blocks(const GemmShape& p, const GemmLaunch& L) {
  if (!p.fast || L.nsplit != 1 || p.ones_col || p.nup || p.scC || p.gh != 1 || p.transA) return 0;
  return L.bm == 64 && L.bn == 64 ? L.tiles_m * L.tiles_n * p.G : 0;
}

// up to four planned problems in one launch: waves / ring depth for the combined grid as a single
// problem's launch would get them, from the shortest k-loop.  (Quirk, kept: no KW = 4 arm -- the
// multi kernel has no such instantiation; and no bias-column / split guard, which multi_blocks
// has already applied.)  Problem i then runs cdiv(nk64_i, kw) k-tiles per k-group.
inline GemmLaunch plan_multi(int total_blocks, int min_nk64, const GemmKnobs& k) {
  GemmLaunch L{};
  L.path = PATH_TILE; L.bm = L.bn = 64; L.nsplit = 1; L.kt_per_split = min_nk64;
  tile_waves(L, total_blocks, min_nk64, k.kw < 2 ? k.kw : 2, true);
  return L;
}

// one problem (weight gradient) of a grouped launch: tile per side, its split and its block count
inline GemmLaunch plan_grouped(int G, int M, int nb, int K, int splitk, const GemmKnobs& k) {
  GemmLaunch L{};
  const KSplit ks = split_k((int)cdiv(K, FAST_BK), splitk > 0 ? splitk : grouped_split(K, k));
  L.path = PATH_TILE; L.kt_per_split = ks.kt; L.nsplit = ks.n;
  L.bm = tile_dim(M); L.bn = tile_dim(nb);
  L.tiles_m = (int)cdiv(M, L.bm); L.tiles_n = (int)cdiv(nb, L.bn);
  L.grid_x = (unsigned)(L.tiles_m * L.tiles_n * G * L.nsplit);
  return L;
}

}  // namespace gemmplan
