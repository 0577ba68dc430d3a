// Prints the launch plan gemm_plan.h computes for every case of a table (tests/golden/gemm_plans.tsv).
//   gemm_plan_dump <table.tsv>
// A case line holds 29 tab-separated input columns (any further columns are ignored):
//   kind G M N K tA tB ones dtype fast splitk a2 row_ln ln_bwd scC nup gh tile_only
//   GEMM_TILES GEMM_SMALLK GEMM_T128 GEMM_SPLITKW GEMM_KW GEMM_MID GEMM_STREAM GEMM_STREAM_K
//   GEMM_STREAM_BPC GROUPED_KT num_cu
// and one output line has the 16 GemmLaunch columns
//   path bm bn ns kw nsplit kt tiles_m tiles_n grid_x grid_y grid_z block red_zl red_grid_x red_grid_y
// Lines starting with '#' are skipped.
#include "../../rgbx_semantic_segmentation_amd/csrc/gemm_plan.h"

#include <stdio.h>
#include <string.h>

using namespace gemmplan;

int main(int argc, char** argv) {
  FILE* f = argc == 2 ? fopen(argv[1], "r") : nullptr;
  if (!f) {
    fprintf(stderr, "usage: gemm_plan_dump <table.tsv>\n");
    return 2;
  }
  char line[1024];
  int lineno = 0;
  while (fgets(line, sizeof(line), f)) {
    ++lineno;
    if (line[0] == '#' || line[0] == '\n') continue;
    char kind[16];
    int v[28];
    int n = sscanf(line, "%15s", kind) == 1 ? 0 : -1;
    const char* p = line;
    for (; n >= 0 && n < 28; ++n) {
      p = strchr(p, '\t');
      if (!p || sscanf(++p, "%d", &v[n]) != 1) break;
    }
    if (n != 28) {
      fprintf(stderr, "line %d: expected a kind and 28 integer columns\n", lineno);
      return 1;
    }
    GemmShape s;
    s.G = v[0]; s.M = v[1]; s.N = v[2]; s.K = v[3]; s.transA = v[4]; s.transB = v[5]; s.ones_col = v[6]; s.dtype = v[7];
    s.fast = v[8]; s.splitk = v[9]; s.a2 = v[10]; s.row_ln = v[11]; s.ln_bwd = v[12]; s.scC = v[13]; s.nup = v[14];
    s.gh = v[15]; s.tile_only = v[16];
    GemmKnobs k;
    k.tiles = v[17]; k.smallk = v[18]; k.t128 = v[19]; k.splitkw = v[20]; k.kw = v[21]; k.mid = v[22]; k.stream = v[23];
    k.stream_k = v[24]; k.stream_bpc = v[25]; k.grouped_kt = v[26];
    const int num_cu = v[27];
    GemmLaunch L{};
    if (!strcmp(kind, "gemm")) {
      L = plan_gemm(s, k, num_cu);
    } else if (!strcmp(kind, "plan")) {
      L.grid_x = (unsigned)multi_blocks(s, plan_gemm(s, k, num_cu));
    } else if (!strcmp(kind, "multi")) {
      L = plan_multi(s.M, s.K, k);
    } else if (!strcmp(kind, "split")) {
      L.nsplit = default_split(s.G, s.M, s.N, s.K, s.ones_col, s.dtype, k);
    } else if (!strcmp(kind, "grouped")) {
      L.nsplit = grouped_split(s.K, k);
    } else if (!strcmp(kind, "gpack")) {
      L = plan_grouped(s.G, s.M, s.ones_col ? s.N - 1 : s.N, s.K, s.splitk, k);
    } else {
      fprintf(stderr, "line %d: unknown kind '%s'\n", lineno, kind);
      return 1;
    }
    printf("%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%u\t%u\t%u\t%u\t%d\t%u\t%u\n", L.path, L.bm, L.bn, L.ns, L.kw, L.nsplit,
           L.kt_per_split, L.tiles_m, L.tiles_n, L.grid_x, L.grid_y, L.grid_z, L.block, L.red_zl, L.red_grid_x,
           L.red_grid_y);
  }
  fclose(f);
  return 0;
}
