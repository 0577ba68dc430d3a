"""The constructions of tests/rectify_cases.py hold on the references and the fp32 emulation alone (CPU, no
kernel): the tables reach every variant of the combine kernels, a partly filled second chunk and a grid wrap exist
for each kernel, the host-side selection is restated as csrc/frm.hip has it, and every exact case is exact: the
fp64 result is representable where the module says so, and the fp32 evaluation equals it bit for bit under both
summation orders."""
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rectify_cases as rc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rgbx_semantic_segmentation_amd", "csrc")
TPRS = {4, 8, 16, 32, 64}


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def same(a, b):
    return torch.equal(a.double(), b.double())


# ------------------------------------------------------------------------------- the tables
def test_tables_reach_every_combine_variant():
    for dts in ((rc.FP32,), (rc.BF16,), (rc.FP16,)):
        cases = [c for c in rc.FRM_CASES if c.dtype in dts]
        assert {c.tpr for c in cases} == TPRS, dts                              # combine_fwd_kernel<T, TPR>
        assert {c.tpr for c in cases if c.bwd} == TPRS, dts                     # combine_bwd_kernel<T, TPR, MCH>
        assert {c.mch for c in cases if c.bwd} == {1, 2}, dts
        assert {(c.tpr, c.mch) for c in cases if c.bwd} == {(t, 1) for t in TPRS} | {(64, 2)}
        assert any(c.partial_second_chunk for c in cases if c.bwd), dts
    assert any(c.fwd_wraps for c in rc.FRM_CASES) and any(c.bwd_wraps and c.bwd for c in rc.FRM_CASES)
    assert any(c.fwd_wraps and c.dtype == rc.FP32 for c in rc.FRM_CASES)
    # the shapes the kernels are asked for
    want = {rc.BF16: {8, 32, 64, 128, 160, 256, 320, 512, 768, 1024}, rc.FP32: {4, 32, 64, 128, 160, 256, 320, 512}}
    want[rc.FP16] = want[rc.BF16]
    for dt, cs in want.items():
        assert {c.C for c in rc.FRM_CASES if c.dtype == dt} >= cs
        for C in cs:
            assert len([c for c in rc.FRM_CASES if c.dtype == dt and c.C == C]) >= 2
    assert {c.B for c in rc.FRM_CASES} >= {1, 3, 8}
    for c in rc.FRM_CASES:
        if not (c.fwd_wraps or c.bwd_wraps):
            assert c.N in (1, c.rpb - 1, c.rpb + 1, 67), c.name
    for t in TPRS:
        assert {1, 67} <= {c.N for c in rc.FRM_CASES if c.tpr == t}
        assert {c.N for c in rc.FRM_CASES if c.tpr == t} & {256 // t - 1, 256 // t + 1}
    # a block of the forward whose rows straddle two images
    assert any(c.B == 3 and c.N == 67 and c.N % c.rpb for c in rc.FRM_CASES)
    names = [c.name for c in rc.FRM_CASES]
    assert len(set(names)) == len(names)
    wraps = {c.name: (c.dtype, c.C, c.B * c.N, c.N) for c in rc.FRM_CASES if c.fwd_wraps or c.bwd_wraps}
    assert (rc.BF16, 512, 2 * 1031, 1031) in wraps.values() and (rc.BF16, 32, 16391, 16391) in wraps.values()
    assert any(v[:3] == (rc.BF16, 512, 16389) for v in wraps.values())
    assert any(v[:3] == (rc.BF16, 32, 262149) for v in wraps.values())
    for c in rc.FRM_CASES:                         # each case moves under 100 MB on the device
        esz = 4 if c.dtype == rc.FP32 else 2
        assert (9 if c.bwd else 5) * c.B * c.N * c.C * esz < 100e6, c.name


def test_pool_bwd_and_ifrm_tables():
    for dt in rc.DTYPES:
        cs = {c.C for c in rc.POOL_BWD_CASES if c.dtype == dt}
        assert cs >= ({4, 160, 512} if dt == rc.FP32 else {8, 160, 512, 1024})
    assert {c.nslice for c in rc.POOL_BWD_CASES} == {1, 5, 16}
    assert {c.B for c in rc.POOL_BWD_CASES if c.wraps} >= {1, 8}
    for c in rc.POOL_BWD_CASES:
        V = rc.vec_width(c.dtype)
        assert rc.pool_bwd_nblk(c.B, c.N, c.C, V) == min(-(-c.N // rc.rpb_of(c.C, V)), -(-512 // (2 * c.B)))
        if c.kind == "exact":
            assert c.N & (c.N - 1) == 0
        part, am, dx0 = rc.pool_bwd_inputs(c)
        assert (am == rc.NO_ARGMAX).sum() == 2 and (am == 0).any() and (am == c.N - 1).any()
        if c.N > 2:
            assert ((am > 0) & (am < c.N - 1)).any()
    assert {(r[1], r[0]) for r in rc.IFRM_RUNS} >= {(C, dt) for dt in rc.DTYPES for C in (rc.vec_width(dt), 32, 160, 320, 512)}
    assert {r[3] for r in rc.IFRM_RUNS} == {1, 15, 16, 17, 67} and {r[2] for r in rc.IFRM_RUNS} == {1, 3}


def test_host_selection_is_the_source():
    """the restated constants are those of the kernels' source text"""
    frm, ifrm = _src("frm.hip"), _src("ifrm.hip")
    assert "int tpr = 4;" in frm and "while (tpr < C / V && tpr < 64) tpr <<= 1;" in frm
    assert "return nb < 256 ? nb : 256;" in frm and "g < 4096 ? (g > 0 ? g : 1) : 4096" in frm
    assert "const long want = (512 + 2 * B - 1) / (2 * B);" in frm
    assert "if (C / V <= tpr) CMX_CB(1);" in frm
    assert re.search(r"constexpr int NSLICE = (\d+);", frm).group(1) == str(rc.NSLICE)
    assert re.search(r"constexpr int SLICE_MAX = (\d+);", frm).group(1) == str(rc.SLICE_MAX)
    assert re.search(r"constexpr int PPB = (\d+);", ifrm).group(1) == str(rc.IFRM_PPB)
    assert rc.row_lanes(8, 8) == 4 and rc.row_lanes(160, 8) == 32 and rc.row_lanes(320, 8) == 64
    assert rc.row_lanes(160, 4) == 64 and rc.mch(320, 4) == 2 and rc.mch(256, 4) == 1 and rc.mch(768, 8) == 2
    assert rc.combine_nblk(1031, 512, 8) == 256 and rc.combine_nblk(67, 512, 8) == 17
    assert rc.rows_grid(16389, 4) == 4096 and rc.rows_grid(0, 4) == 1 and rc.rows_grid(9, 4) == 3
    assert rc.pool_bwd_nblk(8, 133, 512, 8) == 32 and rc.pool_bwd_nblk(1, 1031, 512, 8) == 256


# ------------------------------------------------------------------------------- FRM combine
EXACT_FRM = [(c, k) for c, k in rc.FRM_RUNS if k == "exact"] + \
    [(c, "pos") for c in rc.FRM_POS]


@pytest.mark.parametrize("case,kind", EXACT_FRM, ids=[rc.frm_run_id(r) for r in EXACT_FRM])
def test_frm_exact_cases_are_exact(case, kind):
    inp = rc.frm_inputs(case, kind)
    ref, e = rc.frm_expected(case, kind)
    dt = case.dtype
    assert not e
    for n in ("x", "h", "dout"):
        assert same(inp[n].to(dt), inp[n])
    assert torch.equal(ref["sw"], torch.full_like(ref["sw"], 0.5))
    assert same(ref["out"].to(dt), ref["out"])                     # round-trips through the output type
    if kind == "exact":
        assert (inp["h"] <= 0).all() and (inp["h"] < 0).any()
        z = inp["h"] == 0
        assert z.any() and torch.signbit(inp["h"][z]).all()        # the zeros are -0.0
    else:
        assert (inp["h"] > 0).all() and not inp["w2"].any()
    for order in rc.ORDERS:
        for form in rc.FORMS:
            sw, out = rc.frm_fwd(*(inp[k].float() for k in ("x", "cw", "h", "w2", "b2")), order=order, form=form)
            assert same(sw, ref["sw"]) and same(out, ref["out"]), (order, form)
    if not case.bwd or kind == "pos":
        return
    hb = rc.frm_bwd_h(case, kind)
    z = hb == 0
    assert torch.signbit(hb[z]).any() and not torch.signbit(hb[z]).all()      # +0.0 and -0.0
    assert not ref["dh"][z].any()
    assert set(inp["sw"].unique().tolist()) <= {0.0, 0.25, 0.5, 0.75, 1.0}
    assert same(ref["dx"].to(dt), ref["dx"])
    for n in rc.FRM_BWD_OUT:
        assert same(ref[n].float(), ref[n]), n
    # every sum below 2^24 units of its terms' spacing, in any order
    d1, d2, x1, x2 = inp["dout"][0], inp["dout"][1], inp["x"][0], inp["x"][1]
    assert rc.abs_sums_exact(d1 * x2, 1, 1.0) and rc.abs_sums_exact(d2 * x1, 1, 1.0)
    assert rc.abs_sums_exact(d1 * x2, -1, 1.0) and rc.abs_sums_exact(d2 * x1, -1, 1.0)
    r = hb.clamp_min(0.0)
    for g_, q in ((0, d2 * x1), (1, d1 * x2)):
        s = inp["sw"][..., g_]
        gg = 0.5 * q.sum(-1) * s * (1 - s)
        assert rc.abs_sums_exact((gg[..., None] * r).reshape(-1, case.C), 0, 2.0 ** -5)
        assert rc.abs_sums_exact(gg.reshape(-1), 0, 2.0 ** -5)
    for order in rc.BWD_ORDERS:
        got = rc.frm_bwd(*(t.float() for t in (inp["dout"], inp["x"], inp["cw"], inp["sw"], hb, inp["w2"])), order=order,
                         V=case.V)
        for n, v in zip(rc.FRM_BWD_OUT, got):
            assert same(v, ref[n]), (n, order)


def test_frm_gauss_preactivations_and_yardstick():
    print("\nE_emul FRM combine (fp32 emulation vs fp64)")
    for case, kind in rc.FRM_RUNS:
        if kind != "gauss":
            continue
        inp = rc.frm_inputs(case, kind)
        z = (inp["h"].clamp_min(0.0) @ inp["w2"].t()) + inp["b2"]
        assert z.abs().max() <= rc.ZMAX, case.name
        _, e = rc.frm_expected(case, kind)
        print(f"{case.name:28s} " + " ".join(f"{n} {v:.1e}" for n, v in e.items()))
        for n, v in e.items():
            assert v == v and v <= 1.01 * rc.out_ulp(n, case.dtype) + 1e-4, (case.name, n, v)


@pytest.mark.parametrize("dtype", rc.DTYPES)
def test_dout2_pairs_need_the_rounding(dtype):
    """the pairs' sums are not all representable, some are ties, and a sum carried unrounded in fp32 or
    rounded twice differs from the sum rounded once"""
    d, d2, s = rc.dout2_tensors(dtype, (4096,), rc.gen("dout2", dtype))
    exact = d.double() + d2.double()
    if dtype != rc.FP32:
        assert (s.double() != exact).any()                                  # the rounding is visible
        assert same(s, exact.float().to(dtype))                            # (fp32 holds these sums exactly)
        # ties among them: the exact sum lies halfway between two neighbours of T
        spacing = torch.finfo(dtype).eps * 2.0 ** exact.abs().log2().floor()
        assert ((exact - s.double()).abs() == spacing / 2).any()
        want = {rc.BF16: (256.0, 1.0), rc.FP16: (2048.0, 1.0)}[dtype]
        assert want in rc.DOUT2_PAIRS[dtype]
    else:
        assert same(s, exact.float())


# ------------------------------------------------------------------------------- pooling backward, GEMV pair
@pytest.mark.parametrize("case", [c for c in rc.POOL_BWD_CASES if c.kind == "exact"], ids=lambda c: c.name)
def test_pool_bwd_exact_cases(case):
    part, am, dx0 = rc.pool_bwd_inputs(case)
    ref, e = rc.pool_bwd_expected(case)
    assert e == 0.0 and same(ref.to(case.dtype), ref)
    assert torch.equal(part, part.round()) and abs(part).max() * case.nslice < 2 ** 24
    for order in rc.ORDERS:
        assert same(rc.pool_bwd_formula(part.float(), am, dx0.float(), order), ref)


def test_pool_bwd_no_argmax_channel_gets_no_max_gradient():
    case = rc.POOL_BWD_CASES[0]
    part, am, dx0 = rc.pool_bwd_inputs(case)
    ref, _ = rc.pool_bwd_expected(case)
    b, k = (am == rc.NO_ARGMAX).nonzero()[0].tolist()
    g, c = divmod(k, case.C)
    avg = part.sum(0)[b, k] / case.N
    assert torch.equal(ref[g, b, :, c], dx0[g, b, :, c] + avg)


@pytest.mark.parametrize("case", [c for c in rc.LIN_FWD_CASES if c.kind == "exact"], ids=lambda c: c.name)
def test_linear_fwd_exact_cases(case):
    x, w, b = rc.lin_fwd_inputs(case)
    ref, _ = rc.lin_fwd_expected(case)
    assert same(ref.float(), ref) and (x.abs() @ w.abs().t()).max() < 2 ** 24
    for order in rc.ORDERS:
        for form in rc.FORMS:
            assert same(rc.linear_fwd(x.float(), w.float(), rc.work(b, rc.FP32), case.act, order, form), ref)


def test_linear_tables():
    f = rc.LIN_FWD_CASES
    assert {c.M for c in f} == {1, 3, 8} and {c.K for c in f} == {4, 128, 1028, 2048}
    assert {c.Nout for c in f} == {1, 5, 4096} and {c.act for c in f} == {"none", "relu", "sigmoid"}
    assert any(not c.bias for c in f) and any(c.M * c.K * 4 == 64 * 1024 for c in f)
    b = rc.LIN_BWD_CASES
    assert {c.K for c in b} == {1, 63, 65, 2048} and {c.Nout for c in b} == {10, 4096} and {c.M for c in b} == {8}
    assert {c.nslice for c in b} == {1, 2, 7, 75, 256} and {c.accumulate for c in b} == {0, 1}
    assert any(not c.db for c in b) and any(not c.dxp for c in b)
    assert {c.act for c in b} == {"none", "relu", "sigmoid"}
    assert -(-4096 // rc.NSLICE) == rc.SLICE_MAX and -(-10 // rc.NSLICE) == 1          # rows == SLICE_MAX; slices 10 .. 15 empty
    for c in b:
        if c.act == "relu":
            assert (rc.lin_bwd_inputs(c)[1] == 0).any()


@pytest.mark.parametrize("case", [c for c in rc.LIN_BWD_CASES if c.kind == "exact"], ids=lambda c: c.name)
def test_linear_bwd_exact_cases(case):
    part, y, x, w, dw0, db0 = rc.lin_bwd_inputs(case)
    ref, _ = rc.lin_bwd_expected(case)
    dy = part.abs().sum(0)
    assert (dy @ w.abs()).max() < 2 ** 22 and all(same(r.float(), r) for r in ref)
    for order in rc.ORDERS:
        _, dx, dw, db = rc.linear_bwd(part.float(), y.float(), x.float(), w.float(), case.act, order)
        if case.accumulate:
            dw, db = dw + dw0.float(), db + db0.float()
        assert same(dx, ref[0]) and same(dw, ref[1]) and same(db, ref[2]), order


# ------------------------------------------------------------------------------- FFM context
@pytest.mark.parametrize("D,B,H", rc.FFM_SHAPES)
def test_ffm_exact_kinds(D, B, H):
    for dt in rc.DTYPES:
        kv, sc, ref, _ = rc.ffm_fwd_expected(D, B, H, "const", dt)
        assert torch.equal(ref, torch.full_like(ref, 1.0 / D))
        kv1, sc1, ref1, _ = rc.ffm_fwd_expected(D, B, H, "onehot", dt)
        assert set(ref1.unique().tolist()) == {0.0, 1.0} and torch.equal(ref1.sum(-2), torch.ones_like(ref1.sum(-2)))
        for order in rc.ORDERS:
            for form in rc.FORMS:
                assert same(rc.ffm_fwd(kv.float(), sc, order, form), ref)
                assert same(rc.ffm_fwd(kv1.float(), sc1, order, form), ref1)
        ctx, dctx, s, da, e = rc.ffm_bwd_expected(D, B, H, "exact", dt)
        assert e == 0.0 and s == 0.25 and same(da.float(), da)
        for order in rc.ORDERS:
            assert same(rc.ffm_bwd(ctx.float(), dctx.float().flip(0), s, order), da)
    kv = rc.ffm_fwd_inputs(D, B, H, "gauss")
    flat = kv.reshape(-1, D * D)
    assert len({tuple(r[:4].tolist()) for r in flat}) == flat.shape[0]        # every (g, b, head) its own matrix
    big = rc.ffm_fwd_inputs(D, B, H, "large") * 0.25
    assert 5000 < big.abs().max() <= 10000 and torch.equal(big, big.round())
    _, sc, ref, e = rc.ffm_fwd_expected(D, B, H, "large", rc.FP32)
    assert torch.isfinite(ref).all() and (ref.sum(-2) - 1).abs().max() < 1e-12 and e["ctx"] < 1e-5


# ------------------------------------------------------------------------------- row LayerNorm, IFRM combine
@pytest.mark.parametrize("R,C", rc.ROWLN_SHAPES)
def test_rowln_constructions(R, C):
    x, gamma, beta, dy = rc.rowln_inputs(R, C, "const")
    ref, e, _ = rc.rowln_expected(R, C, "const")
    for order in rc.ORDERS:
        y, mu, rs = rc.rowln_fwd(x.float(), gamma.float(), beta.float(), rc.ROWLN_EPS, order)
        assert same(y, beta.expand(R, C)) and same(mu, x[:, 0])
        assert ((rs.double() * rc.ROWLN_EPS ** 0.5 - 1).abs() <= rc.ULP32).all()
    for kind in rc.ROWLN_KINDS:
        x, gamma, beta, dy = rc.rowln_inputs(R, C, kind)
        ref, e, _ = rc.rowln_expected(R, C, kind)
        assert R * 4 < 2 ** 24 and e["dbeta"] == 0.0 and torch.equal(ref["dbeta"], ref["dbeta"].round())
        print(f"rowln R{R} C{C} {kind}: " + " ".join(f"{n} {v:.1e}" for n, v in e.items()))
        assert all(v == v and v < 1e-4 for v in e.values())
    # the offset kind shows a one-pass variance wherever E[x^2] is not exact in fp32
    if C >= 64:
        x, gamma, beta, _ = rc.rowln_inputs(R, C, "offset")
        ref, e, _ = rc.rowln_expected(R, C, "offset")
        bnd = rc.bound(e["rstd"], rc.ULP32)
        sig = max(rc.tenerr(rc.rowln_fwd(x.float(), gamma.float(), beta.float(), rc.ROWLN_EPS, o, one_pass=True)[2],
                            ref["rstd"]) for o in rc.ORDERS)
        print(f"rowln R{R} C{C} one-pass rstd error {sig:.2e} bound {bnd:.2e}")
        assert sig > 10 * bnd or R == 1, (sig, bnd)


EXACT_IFRM = [r for r in rc.IFRM_RUNS if r[4] == "exact"]


@pytest.mark.parametrize("run", EXACT_IFRM, ids=[rc.ifrm_run_id(r) for r in EXACT_IFRM])
def test_ifrm_exact_cases(run):
    dt = run[0]
    inp = rc.ifrm_inputs(*run)
    ref, e = rc.ifrm_expected(*run)
    assert not e and same(inp["sw"].to(dt), inp["sw"])
    assert same(ref["out"].to(dt), ref["out"]) and same(ref["dx"].to(dt), ref["dx"])
    for n in rc.IFRM_OUT:
        assert same(ref[n].float(), ref[n]), n
    for order in rc.ORDERS:
        f = {k: v.float() for k, v in inp.items()}
        got = (rc.ifrm_fwd(f["x"], f["cw"], f["sw"], f["lc"], f["ls"]),) + \
            rc.ifrm_bwd(f["dout"], f["x"], f["cw"], f["sw"], f["lc"], f["ls"], order)
        for n, v in zip(rc.IFRM_OUT, got):
            assert same(v, ref[n]), (n, order)
