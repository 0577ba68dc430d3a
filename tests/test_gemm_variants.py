"""Ties the exact-result GEMM cases (tests/gemm_cases.py, run on the GPU by
tests/test_gpu_gemm_exact.py) to the kernels they are meant to run: csrc/gemm_plan.h, built with the
host compiler as tests/test_gemm_plan.py builds it, must plan every case at 256 CUs and the case's
knobs as exactly the variant the case names; and every tile, multi and reducer kernel the sources
instantiate must be named by at least one case, so a kernel added later without an exact case
fails here, without a GPU.  Also checks, in fp32 on the CPU, that the GELU bound of the GPU test
holds for the fp32 restatement of cmx_erf over the cases' whole pre-activation range."""
import os
import re
import shutil
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_cases as gc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rgbx_semantic_segmentation_amd", "csrc")
OUT = "path bm bn ns kw nsplit kt tiles_m tiles_n grid_x grid_y grid_z block red_zl red_grid_x red_grid_y".split()


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    """plan(rows) -> one dict of GemmLaunch columns per input row"""
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler (c++ / g++ / clang++) on PATH"
    tmp = tmp_path_factory.mktemp("gemm_variants")
    exe = str(tmp / "gemm_plan_dump")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "host", "gemm_plan_dump.cpp"),
                    "-o", exe], check=True)

    def run(rows):
        table = str(tmp / "rows.tsv")
        with open(table, "w") as f:
            f.write("\n".join(rows) + "\n")
        out = subprocess.run([exe, table], check=True, capture_output=True, text=True).stdout.splitlines()
        assert len(out) == len(rows)
        return [dict(zip(OUT, map(int, ln.split("\t")))) for ln in out]
    return run


def planned(plan, G, M, N, K, tA, tB, epi, dtype, fast, splitk, knobs, row_ln=0, tile_only=0):
    """the launch of one problem as the Python wrapper gets it: cmx_gemm_splitk first (a `split`
    row), then the launch with that split (a `gemm` row)"""
    e = gc.EPIS[epi]
    ones, a2 = int(bool(e.get("dbias"))), int(bool(e.get("a2")))
    kw = dict(tA=tA, tB=tB, ones=ones, dtype=gc.DTYPE_CODE[dtype], fast=fast, a2=a2, knobs=knobs)
    if splitk <= 0:
        splitk = plan([gc.plan_row("split", G, M, N + ones, K, **kw)])[0]["nsplit"]
    return plan([gc.plan_row("gemm", G, M, N + ones, K, splitk=splitk, row_ln=row_ln, tile_only=tile_only, **kw)])[0]


def as_variant(L):
    ns = L["ns"] if L["path"] == gc.PATH_TILE else 0
    return gc.Variant(L["path"], L["bm"], L["bn"], ns, L["kw"], L["nsplit"] > 1, L["red_zl"])


def test_every_case_plans_to_its_variant(plan):
    bad = []
    for r in gc.runs():
        c = r.case
        got = as_variant(planned(plan, c.G, c.M, c.N, c.K, c.tA, c.tB, r.epi, r.dtype, c.fast, c.splitk, c.knobs))
        if got != r.variant:
            bad.append(f"{gc.run_id(r)}: planned {got}, the case names {r.variant}")
    c = gc.LN_CASE
    got = as_variant(planned(plan, c.G, c.M, c.N, c.K, 0, 0, c.epis[0], "bfloat16", 1, 1, c.knobs, row_ln=1))
    if got != c.variant:
        bad.append(f"{c.name}: planned {got}, the case names {c.variant}")
    assert not bad, "\n".join(bad)


def test_knob_defaults_are_the_headers():
    """the defaults the rows above spell out (gemm_cases.KNOB_DEFAULTS, which the GPU test also
    expects to find set) are GemmKnobs' in gemm_plan.h"""
    with open(os.path.join(CSRC, "gemm_plan.h")) as f:
        src = f.read()
    lb = re.search(r"#define CMX_STREAM_LB (\d+)", src).group(1)
    body = src[src.index("struct GemmKnobs {"):]
    found = re.findall(r"int \w+ = (\w+);\s*// (\w+)", body[:body.index("};")])
    assert {name: int(lb if v == "CMX_STREAM_LB" else v) for v, name in found} == gc.KNOB_DEFAULTS


def multi_plan(plan, mc):
    """(blocks per problem, the combined launch) of a multi case"""
    blocks, nk64 = [], []
    for G, M, N, K, epi in mc.problems:
        sk = plan([gc.plan_row("split", G, M, N, K, tB=mc.tB)])[0]["nsplit"]
        blocks.append(plan([gc.plan_row("plan", G, M, N, K, tB=mc.tB, splitk=sk, tile_only=1)])[0]["grid_x"] if sk == 1 else 0)
        nk64.append((K + 63) // 64)
    return blocks, plan([gc.plan_row("multi", 1, sum(blocks), 0, min(nk64))])[0]


def test_every_multi_case_plans_to_its_variant(plan):
    for mc in gc.MULTI_CASES:
        blocks, L = multi_plan(plan, mc)
        assert all(b > 0 for b in blocks), f"{mc.name}: a problem is not eligible for the multi launch: {blocks}"
        assert 2 <= len(blocks) <= 4
        assert (L["ns"], L["kw"]) == (mc.ns, mc.kw), f"{mc.name}: planned NS {L['ns']} KW {L['kw']} over {sum(blocks)} blocks"


def test_every_instantiated_kernel_has_an_exact_case():
    """the CMX_GEMM_TILE list of launch_tile, the CMX_GEMM_MULTI_W list of cmx_gemm_multi and the
    reducer widths of launch_reduce against the variants the cases name (each of which the tests
    above pin to the plan)"""
    with open(os.path.join(CSRC, "gemm_kernels.h")) as f:
        kern = f.read()
    with open(os.path.join(CSRC, "gemm.hip")) as f:
        hip = f.read()
    tiles = {tuple(map(int, m)) for m in re.findall(r"CMX_GEMM_TILE\((\d+),\s*(\d+),\s*(\d+),\s*(\d+)\)", kern)}
    multis = {tuple(map(int, m)) for m in re.findall(r"CMX_GEMM_MULTI_W\((\d+),\s*(\d+)\)", hip)}
    body = kern[kern.index("void launch_reduce("):]
    widths = {int(m) for m in re.findall(r"splitk_reduce_kernel<T,\s*(\d+)>", body[:body.index("\n}\n")])}
    assert tiles and multis and widths, "the instantiation lists were not found in the sources"
    variants = [r.variant for r in gc.runs()] + [gc.LN_CASE.variant]
    named_tiles = {(v.bm, v.bn, v.ns, v.kw) for v in variants if v.path == gc.PATH_TILE}
    named_widths = {v.red_zl for v in variants if v.red_zl}
    named_multis = {(mc.ns, mc.kw) for mc in gc.MULTI_CASES}
    assert not tiles - named_tiles, f"tile kernels (BM, BN, NS, KW) without an exact case: {sorted(tiles - named_tiles)}"
    assert not multis - named_multis, f"multi kernels (NS, KW) without an exact case: {sorted(multis - named_multis)}"
    assert not widths - named_widths, f"reducer widths without an exact case: {sorted(widths - named_widths)}"
    assert any(v.path == gc.PATH_STREAM for v in variants) and any(v.path == gc.PATH_GENERIC for v in variants)
    # a case naming a kernel that does not exist would be a stale table
    assert named_tiles <= tiles and named_multis <= multis and named_widths <= widths
    print("covered:", sorted(named_tiles), sorted(named_multis), sorted(named_widths))


def test_gelu_bound_holds_for_the_fp32_restatement():
    """gemm_cases.gelu_delta against the fp32 restatement of the kernels' GELU (cmx_erf's
    coefficients parsed from cmx_common.h as test_oracle_kats.py::test_fast_erf_table does, the
    reciprocal correctly rounded) on every multiple of 1/4 a GELU case's pre-activation can take."""
    import numpy as np
    import torch
    with open(os.path.join(CSRC, "cmx_common.h")) as f:
        src = f.read()
    body = src[src.index("float cmx_erf(float x)"):]
    body = body[:body.index("return x * p")]
    lits = [np.float32(v) for v in re.findall(r"(-?\d\.\d+e-\d+)f", body)]
    assert len(lits) == 12
    f = np.float32
    vmax = gc.gelu_vmax()
    v = (np.arange(-4 * vmax, 4 * vmax + 1, dtype=np.float64) / 4).astype(f)
    x = v * f(0.70710678118654752)
    xc = np.clip(x, f(-4), f(4))
    x2 = xc * xc
    p = np.full_like(x2, lits[0])
    for a in lits[1:7]:
        p = p * x2 + a
    q = np.full_like(x2, lits[7])
    for b in lits[8:]:
        q = q * x2 + b
    erf32 = xc * p * (f(1) / q)
    y = f(0.5) * v * (f(1) + erf32)
    assert y.dtype == np.float32
    v64 = torch.from_numpy(v.astype(np.float64))
    ref = (0.5 * v64 * (1 + torch.erf(v64 * 0.5 ** 0.5))).numpy()
    err = np.abs(y.astype(np.float64) - ref)
    bound = gc.gelu_delta(v.astype(np.float64))
    i = int(np.argmax(err - bound))
    assert (err <= bound).all(), f"v = {v[i]}: |y - ref| = {err[i]:.3e} > delta = {bound[i]:.3e}"
