"""The constructions of tests/norm_cases.py hold on the references and the fp32 emulation alone (CPU, no
kernel): the stated exact results are exact, the kinds decide what they are meant to decide (the other
eps, a one-pass variance), every yardstick stays below those signals, and every LayerNorm case lands on
the launch plan it names (csrc/ln_plan.h through tests/host/ln_plan_dump.cpp, built by the host compiler)
with the table covering every instantiation of layernorm.hip.  Prints E_emul of every case."""
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import norm_cases as nc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LN_IDS = [c.name for c in nc.LN_CASES]
BN_IDS = [c.name for c in nc.BN_CASES]


def other_eps(eps, pair):
    return pair[1] if eps == pair[0] else pair[0]


# ------------------------------------------------------------------------------- the plan
@pytest.fixture(scope="module")
def ln_plans(tmp_path_factory):
    """{(R, G, C, dtype code): (fwd (tpr, nch, rpt), fwd grid, bwd (tpr, nch, rpt), bwd grid, nb, bytes)}"""
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler (c++ / g++ / clang++) on PATH"
    exe = str(tmp_path_factory.mktemp("ln_plan") / "ln_plan_dump")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "host", "ln_plan_dump.cpp"),
                    "-o", exe], check=True)
    keys = [(c.R, c.G, c.C, nc.dtype_code(dt)) for c in nc.LN_CASES for dt in c.dtypes]
    keys += [(R, 1, C, d) for R, C, d in EXTRA_PLANS]
    out = subprocess.run([exe], input="".join("%d %d %d %d\n" % k for k in keys), check=True, capture_output=True,
                         text=True).stdout.splitlines()
    assert len(out) == len(keys)
    plans = {}
    for k, ln in zip(keys, out):
        v = [int(t) for t in ln.split()]
        plans[k] = (tuple(v[0:3]), tuple(v[3:5]), tuple(v[5:8]), tuple(v[8:10]), v[10], v[11])
    return plans


# either side of every threshold of the policy: (R, C, dtype code) -> (fwd, bwd) instantiation
EXTRA_PLANS = {
    (65535, 32, 1): ((4, 1, 1), (4, 1, 2)), (65536, 32, 1): ((4, 1, 4), (4, 1, 2)),      # forward rpt 4: R G >= 1024 rpb
    (32768, 32, 1): ((4, 1, 1), (4, 1, 1)), (32769, 32, 1): ((4, 1, 1), (4, 1, 2)),      # backward rpt 2: R > 512 rpb
    (16384, 128, 1): ((16, 1, 4), (16, 1, 2)), (16383, 128, 1): ((16, 1, 1), (16, 1, 2)),
    (8193, 256, 1): ((32, 1, 1), (32, 1, 1)),                                            # tpr 32: never more than a row
    (100, 512, 0): ((64, 2, 1), (64, 2, 1)), (100, 516, 0): ((64, 4, 1), (64, 4, 1)),    # three chunks run NCH = 4
    (100, 768, 0): ((64, 4, 1), (64, 4, 1)), (100, 772, 0): ((64, 4, 1), (64, 4, 1)),
    (100, 512, 1): ((64, 1, 1), (64, 1, 1)), (100, 520, 2): ((64, 2, 1), (64, 2, 1)),
}


def test_ln_cases_land_on_their_plans(ln_plans):
    for c in nc.LN_CASES:
        for dt in c.dtypes:
            fwd, fgrid, bwd, bgrid, nb, nbytes = ln_plans[(c.R, c.G, c.C, nc.dtype_code(dt))]
            assert (fwd, bwd) == (c.fwd, c.bwd), (c.name, dt, fwd, bwd)
            rpb = 256 // fwd[0]
            assert fgrid == (-(-c.R // (rpb * fwd[2])), c.G) and bgrid == (nb, c.G), c.name
            assert nb == min(512, -(-c.R // rpb)) and nbytes == c.G * nb * 2 * c.C * 4, c.name
    for (R, C, d), want in EXTRA_PLANS.items():
        assert (ln_plans[(R, 1, C, d)][0], ln_plans[(R, 1, C, d)][2]) == want, (R, C, d)


def test_ln_table_covers_every_instantiation():
    """the <TPR, NCH, RPT> lists of layernorm.hip, read from the source, are the plans the table names"""
    with open(os.path.join(ROOT, "rgbx_semantic_segmentation_amd", "csrc", "layernorm.hip")) as f:
        src = f.read()
    lnf = {tuple(int(v) for v in m) for m in re.findall(r"\bLNF\((\d+), (\d+), (\d+)\)", src)}
    lnb = {tuple(int(v) for v in m) for m in re.findall(r"\bLNB\((\d+), (\d+), (\d+)\)", src)}
    assert lnf == set(nc.LN_FWD_PLANS) and len(lnf) == 10
    assert lnb == set(nc.LN_BWD_PLANS) and len(lnb) == 10
    assert {c.fwd for c in nc.LN_CASES} == lnf, sorted(lnf - {c.fwd for c in nc.LN_CASES})
    assert {c.bwd for c in nc.LN_CASES} == lnb, sorted(lnb - {c.bwd for c in nc.LN_CASES})
    assert {(c.fwd, c.bwd) for c in nc.LN_CONTAINMENT} == {(c.fwd, c.bwd) for c in nc.LN_CASES}
    # the shapes the issue names
    h16 = {c.C for c in nc.LN_CASES if c.dtypes == nc.H16 or c.dtypes[0] in nc.H16}
    f32 = {c.C for c in nc.LN_CASES if c.dtypes == nc.F32}
    assert h16 >= {8, 24, 40, 160, 320, 1024} and f32 >= {12, 160, 320, 640, 768, 1024}
    assert {c.G for c in nc.LN_CASES} == {1, 2}
    for C, dts in ((32, nc.H16), (128, nc.H16), (1024, nc.H16), (16, nc.F32), (64, nc.F32), (1024, nc.F32)):
        rpb = 256 // [c for c in nc.LN_CASES if c.C == C and c.dtypes == dts][0].fwd[0]
        assert {c.R for c in nc.LN_CASES if c.C == C and c.dtypes == dts} >= {1, rpb - 1, rpb + 1}, (C, dts)
    assert any(c.bwd[0] >= 32 and c.bwd[2] == 1 and c.R > 512 * (256 // c.bwd[0]) for c in nc.LN_CASES)
    # a block spans two samples, and with G = 2 a sample spans the groups' boundary rows
    assert all(c.rps % (256 // c.fwd[0]) for c in nc.LN_CASES)
    assert any(c.G == 2 and c.R % c.rps and c.rows % c.rps == 0 for c in nc.LN_CASES)


def test_names_unique_and_sizes_small():
    for cases in (nc.LN_CASES, nc.BN_CASES):
        names = [c.name for c in cases]
        assert len(set(names)) == len(names)
    assert max(c.rows * c.C for c in nc.LN_CASES) <= 65573 * 32
    assert max(c.M * c.C for c in nc.BN_CASES) <= 5003 * 136
    # integer gradients: the column sums of dy + dy2 (LayerNorm) and of 2 dy (BatchNorm) stay exact in fp32
    assert max(c.R for c in nc.LN_CASES) * 8 < 2 ** 24 and max(c.M for c in nc.BN_CASES) * 8 < 2 ** 24


# ------------------------------------------------------------------------------ LayerNorm
LN_CONST = [c for c in nc.LN_CASES if "const" in c.kinds]


def test_ln_const_kind_reaches_every_width():
    """the 2 M-element cases hold no const kind; their widths have one in a smaller case of the same dtype"""
    have = {(c.C, dt) for c in LN_CONST for dt in c.dtypes}
    assert have == {(c.C, dt) for c in nc.LN_CASES for dt in c.dtypes}


@pytest.mark.parametrize("case", LN_CONST, ids=[c.name for c in LN_CONST])
def test_ln_const_rows_are_exact_in_the_emulation(case):
    for dt in case.dtypes:
        inp = nc.make_ln_inputs(case, "const", dt)
        for eps in nc.LN_EPS:
            for order in nc.ORDERS:
                y, mu, rs = nc.emulate_ln_fwd(inp, case.G, eps, dt, order)
                beta = inp.beta.to(dt).double()[:, None, :].expand(case.G, case.R, case.C).reshape(-1, case.C)
                assert torch.equal(y, beta), (case.name, dt, order)
                assert torch.equal(mu.double(), inp.x[:, 0]), (case.name, dt, order)          # variance exactly 0:
                assert torch.equal(rs, torch.rsqrt(torch.zeros_like(rs) + eps)), (case.name, dt, order)


@pytest.mark.parametrize("case", nc.LN_CASES, ids=LN_IDS)
def test_ln_integer_sums_and_power_of_two_scales(case):
    dt, eps, kind = case.dtypes[0], nc.LN_EPS[0], case.kinds[0]
    exp = nc.ln_expected(case, kind, dt, eps)
    inp, ref = exp.inp, exp.ref
    for t in (inp.dy, inp.dy2, inp.dres):
        assert torch.equal(t, t.round()) and t.abs().max() <= 4
    assert (inp.dy + inp.dy2).view(case.G, case.R, case.C).abs().sum(1).max() < 2 ** 24
    for variant in ("plain", "all"):
        want = nc.ln_expected_bwd(case, inp, ref, variant)
        assert exp.e[(variant, "dbeta")] == 0.0 and torch.equal(want.dbeta, want.dbeta.round()), case.name
    # dxs == sscale dx on the stored values wherever the sample's scale is 0 or a power of two
    assert (inp.sscale == 1.25).sum() == 1 and set(inp.sscale.tolist()) <= {0.0, 0.5, 1.0, 2.0, 1.25}
    s = inp.sscale[nc.sample_of_row(case)][:, None]
    for order in nc.ORDERS:
        _, mu, rs = nc.emulate_ln_fwd(inp, case.G, eps, dt, order)
        got = nc.emulate_ln_bwd(case, inp, dt, order, mu, rs, "all")
        pow2 = nc.pow2_exact(s, got.dx, dt)
        assert pow2.any() or case.nsamp == 1, case.name
        assert torch.equal(got.dxs[pow2], (s * got.dx)[pow2]), (case.name, order)
    # and the fp64 reference rounds the same way
    want = nc.ln_expected_bwd(case, inp, ref, "all")
    dx = want.dx.to(dt).double()
    pow2 = nc.pow2_exact(s, dx, dt)
    assert torch.equal(want.dxs.to(dt).double()[pow2], (s * dx)[pow2])


def one_pass_blind(case, dt, kind):
    """where a one-pass fp32 variance is legitimately as good as the two-pass one: E[x^2] and mean^2 of these
    few-bit inputs are exact in fp32 at eight values a row, a single row decides by chance, and bf16's offset
    step of 1/2 leaves a variance of 6, whose relative error (5e-5) is no 10 x the bound at every C"""
    return case.C == 8 or case.R == 1 or (dt == nc.BF16 and kind == "offset")


@pytest.mark.parametrize("case", nc.LN_CASES, ids=LN_IDS)
def test_ln_kinds_are_decisive(case):
    for dt in case.dtypes:
        for eps in nc.LN_EPS:
            for kind in case.kinds:
                exp = nc.ln_expected(case, kind, dt, eps)
                if kind == "tiny":
                    swapped = nc.ln_reference(exp.inp, case.G, other_eps(eps, nc.LN_EPS))
                    signal, bnd = nc.rowerr(swapped.y, exp.ref.y), nc.ln_bound(exp, "y", dt)
                    assert signal > 10 * bnd, (case.name, dt, eps, signal, bnd)
                    assert exp.e["y"] < signal
                if kind in ("tiny", "offset") and not one_pass_blind(case, dt, kind):
                    bnd = nc.ln_bound(exp, "rstd", dt)
                    for order in nc.ORDERS:
                        rs = nc.emulate_ln_fwd(exp.inp, case.G, eps, dt, order, one_pass=True)[2]
                        signal = nc.tenerr(rs, exp.ref.rstd)
                        assert signal > 10 * bnd, (case.name, dt, eps, kind, order, signal, bnd)
                        assert exp.e["rstd"] < signal


def test_ln_one_pass_is_caught_in_every_dtype_and_plan():
    """the exemptions of one_pass_blind leave every dtype, and every plan but the single-row ones, a case
    that decides"""
    seen = {(dt, c.bwd) for c in nc.LN_CASES for dt in c.dtypes for kind in ("tiny", "offset")
            if kind in c.kinds and not one_pass_blind(c, dt, kind)}
    assert {dt for dt, _ in seen} == {nc.BF16, nc.FP16, nc.FP32}
    assert {p for _, p in seen} == set(nc.LN_BWD_PLANS)


def test_ln_e_emul_printed_and_rounding_level():
    print("\nE_emul LayerNorm (fp32 emulation vs fp64; y / dx / dxs per row, the rest per tensor; variant all)")
    print(f"{'case':22s} {'dtype':8s} {'eps':6s} {'kind':7s} " + " ".join(f"{n:>8s}" for n in
                                                                         ("y", "mean", "rstd", "dx", "dxs", "dgamma", "dbeta")))
    for case, dt, eps in nc.ln_runs():
        for kind in case.kinds:
            e = nc.ln_expected(case, kind, dt, eps).e
            vals = [e["y"], e["mean"], e["rstd"]] + [e[("all", n)] for n in ("dx", "dxs", "dgamma", "dbeta")]
            print(f"{case.name:22s} {nc.name_of(dt):8s} {eps:<6g} {kind:7s} " + " ".join(f"{v:8.1e}" for v in vals))
            for key, v in e.items():
                name = key[1] if isinstance(key, tuple) else key
                # a rounding-level quantity: the 16-bit store (half a unit of 2^-7 / 2^-10 of the row scale),
                # fp32 sums of up to 1024 terms (offset: x - mean ~ 1 beside x ~ 64), and on the tiny kind
                # the mean's fp32 rounding (2^-24) beside x - mean ~ 2^-10: 2^-14 = 6e-5 of xhat
                cap = 1.01 * nc.ULP[dt] + 1e-4 if name in ("y", "dx", "dxs") else 1e-4
                assert v == v and v <= cap, (case.name, dt, eps, kind, key, v)


# ------------------------------------------------------------------------------ BatchNorm
def test_bn_table_covers_the_issue():
    assert {c.tpr for c in nc.BN_CASES} == {4, 8, 16, 32}
    assert {c.nblk for c in nc.BN_CASES} >= {1, 2, 18, 65, 250, 256}
    assert {c.M for c in nc.BN_CASES} >= {2, 17}
    f32 = {c.C for c in nc.BN_CASES if c.dtypes == nc.F32}
    h16 = {c.C for c in nc.BN_CASES if c.dtypes == nc.H16}
    assert f32 >= {16, 32, 64, 136} and h16 >= {8, 32, 64, 128, 136, 512}
    small = {(c.M, c.C) for c in nc.BN_CASES if c.small}
    assert small == {(M, C) for M in (2, 63, 600) for C in (16, 512)}
    assert all(c.C % 16 == 0 and c.M <= 600 for c in nc.BN_CASES if c.small)
    assert {(c.act, c.res, c.dscale) for c in nc.BN_CASES} == \
        {(a, r, d) for a in ("none", "relu") for r in (False, True) for d in (False, True)}
    assert all(c.M <= 1031 for c in nc.BN_CASES if c.act == "relu")
    for c in nc.BN_SYNC + nc.BN_CONTAINMENT:
        assert c in nc.BN_CASES
    assert len(nc.BN_SYNC) >= 6 and len(nc.BN_CONTAINMENT) == 7


@pytest.mark.parametrize("case", nc.BN_CASES, ids=BN_IDS)
def test_bn_constructions(case):
    for dt in case.dtypes:
        for eps in nc.BN_EPS:
            for kind in case.kinds:
                exp = nc.bn_expected(case, kind, dt, eps)
                inp, ref = exp.inp, exp.ref
                assert torch.equal(inp.dy, inp.dy.round()) and inp.dy.abs().max() <= 4
                if inp.dscale is not None:
                    assert set(inp.dscale.unique().tolist()) <= {0.0, 2.0}
                if case.exact_dbeta:
                    assert torch.equal(ref.dbeta, ref.dbeta.round()) and exp.e["dbeta"] == 0.0, (case.name, dt, kind)
                if case.act == "relu":
                    for training in (True, False):
                        r = nc.bn_expected(case, kind, dt, eps, training).ref
                        pre = nc._bn_pre(inp.x, inp.gamma, inp.beta, inp.res, r.mean, r.invstd)
                        assert pre.abs().min() > nc.RELU_MARGIN / 2, (case.name, dt, kind, training)
                if kind == "const":
                    dyadic = torch.ones(case.C, dtype=torch.bool)
                    dyadic[1:2] = False
                    assert torch.equal(ref.mean[dyadic], inp.x[0][dyadic]) and torch.equal(ref.mean.float().double(), inp.x[0])
                    assert (ref.invstd * eps ** 0.5 - 1).abs().max() < 1e-9
                    # the channel at 0.1: fp64 E[x^2] - mean^2 is rounding noise beside eps, of either sign
                    x1 = inp.x[:, 1]
                    assert ((x1 * x1).mean() - x1.mean() ** 2).abs() < 1e-15 * max(1.0, float(x1[0]) ** 2) * 4
                if kind == "tiny":
                    swapped = nc.bn_reference(case, inp, other_eps(eps, nc.BN_EPS))
                    signal, bnd = nc.rowerr(swapped.y, ref.y, 0), nc.bn_bound(exp, "y", dt)
                    assert signal > 10 * bnd and exp.e["y"] < signal, (case.name, dt, eps, signal, bnd)


def test_bn_e_emul_printed():
    print("\nE_emul BatchNorm (fp32 emulation from fp64 statistics vs fp64; y / dx / dres per channel)")
    for training in (True, False):
        for case, dt, eps in nc.bn_runs():
            for kind in case.kinds:
                e = nc.bn_expected(case, kind, dt, eps, training).e
                print(f"{case.name:24s} {nc.name_of(dt):8s} {eps:<6g} {kind:7s} {'train' if training else 'eval':5s} " +
                      " ".join(f"{n} {v:.1e}" for n, v in e.items()))
                assert all(v == v and v < float("inf") for v in e.values())
                for n in ("mean", "invstd", "rmean", "rvar", "dgamma", "dbeta"):
                    assert e[n] <= 2e-5, (case.name, dt, eps, kind, n, e[n])
