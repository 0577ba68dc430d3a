"""The kernels of csrc/ifrm.hip through the C-ABI: cmx_mul2 / _bwd, cmx_rowln_fwd / _bwd and
cmx_ifrm_combine_fwd / _bwd.  Cases, fp64 references, the fp32 emulation and the bound 2 E_emul + u:
tests/rectify_cases.py.  Every buffer is Guarded, every output starts as the NaN pattern, every launch is made twice
and must give equal bits; every slot of the combine backward's part (nblk, 2C) and lpart (2, nblk) must be written."""
import os
import sys

import pytest
import torch

from rgbx_semantic_segmentation_amd import _lib
from rgbx_semantic_segmentation_amd._lib import call, query, stream, try_call

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rectify_cases as rc  # noqa: E402
from kernel_harness import CODE, Check, Guarded, all_intact, put, twice  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = torch.float32
SHAPE = _lib.CMX_ERR_SHAPE


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_mul2_exact_on_integers(dev, n):
    g = rc.gen("mul2", n)
    a, b, d = rc.ints(g, -9, 9, n), rc.ints(g, -9, 9, n), rc.ints(g, -9, 9, n)
    ad, bd, dd = put(a, F32, dev), put(b, F32, dev), put(d, F32, dev)
    o, da, db = (Guarded((n,), F32, dev) for _ in range(3))
    (g_o,) = twice(lambda: call("cmx_mul2", ad.t, bd.t, o.t, n, stream()), [o])
    g_da, g_db = twice(lambda: call("cmx_mul2_bwd", dd.t, ad.t, bd.t, da.t, db.t, n, stream()), [da, db])
    assert all_intact([ad, bd, dd, o, da, db]), "a guard changed"
    ck = Check("mul2", f"n{n}")
    ck.exact("out", g_o, a * b)
    ck.exact("da", g_da, d * b)
    ck.exact("db", g_db, d * a)
    ck.done()


@pytest.mark.parametrize("kind", rc.ROWLN_KINDS)
@pytest.mark.parametrize("R,C", rc.ROWLN_SHAPES)
def test_rowln(dev, R, C, kind):
    x, gamma, beta, dy = rc.rowln_inputs(R, C, kind)
    ref, e, (mu32, rs32) = rc.rowln_expected(R, C, kind)
    xd, gd, bd, dyd = put(x, F32, dev), put(gamma, F32, dev), put(beta, F32, dev), put(dy, F32, dev)
    y, mean, rstd = Guarded((R, C), F32, dev), Guarded((R,), F32, dev), Guarded((R,), F32, dev)
    fwd = twice(lambda: call("cmx_rowln_fwd", xd.t, gd.t, bd.t, y.t, mean.t, rstd.t, R, C, rc.ROWLN_EPS, stream()),
                [y, mean, rstd])
    mud, rsd = put(mu32, F32, dev), put(rs32, F32, dev)           # the backward's statistics are given
    dx, dg, db = Guarded((R, C), F32, dev), Guarded((C,), F32, dev), Guarded((C,), F32, dev)
    bwd = twice(lambda: call("cmx_rowln_bwd", dyd.t, xd.t, gd.t, mud.t, rsd.t, dx.t, dg.t, db.t, R, C, stream()),
                [dx, dg, db])
    assert all_intact([xd, gd, bd, dyd, y, mean, rstd, mud, rsd, dx, dg, db]), "a guard changed"
    ck = Check("rowln", f"R{R}_C{C}_{kind}")
    for n, got in zip(rc.ROWLN_OUT, fwd + bwd):
        assert not torch.isnan(got).any(), n
        if n == "dbeta" or (kind == "const" and n in ("y", "mean")):
            # integer dy: dbeta is the exact column sum; a constant row: mean == the constant, y == beta
            ck.exact(n, got, ref[n])
            continue
        err, bnd = rc.rowln_err(n, got, ref, R, C, kind), rc.bound(e[n], rc.ULP32)
        rc.report("rowln", ck.case, n, err, bnd)
        if not err <= bnd:
            ck.bad.append((n, err, bnd))
    ck.done()


@pytest.mark.parametrize("run", rc.IFRM_RUNS, ids=[rc.ifrm_run_id(r) for r in rc.IFRM_RUNS])
def test_ifrm_combine(dev, run):
    dt, C, B, N, kind = run
    inp = rc.ifrm_inputs(*run)
    ref, e = rc.ifrm_expected(*run)
    nblk = query("cmx_ifrm_combine_nblk", B, N)
    assert nblk == rc.ifrm_nblk(B, N)                                # the restatement has not drifted
    x, dout, sw = put(inp["x"], dt, dev), put(inp["dout"], dt, dev), put(inp["sw"], dt, dev)
    cw, lc, ls = put(inp["cw"], F32, dev), put(inp["lc"], F32, dev), put(inp["ls"], F32, dev)
    out, dx, dsw = Guarded((2, B, N, C), dt, dev), Guarded((2, B, N, C), dt, dev), Guarded((B, N, 2), dt, dev)
    part, lpart = Guarded((nblk, 2 * C), F32, dev), Guarded((2, nblk), F32, dev)
    (g_out,) = twice(lambda: call("cmx_ifrm_combine_fwd", x.t, cw.t, sw.t, lc.t, ls.t, out.t, B, N, C, CODE[dt], stream()),
                     [out])
    g_dx, g_dsw, g_part, g_lpart = twice(
        lambda: call("cmx_ifrm_combine_bwd", dout.t, x.t, cw.t, sw.t, lc.t, ls.t, dx.t, dsw.t, part.t, lpart.t, B, N, C,
                     CODE[dt], stream()), [dx, dsw, part, lpart])
    assert all_intact([x, dout, sw, cw, lc, ls, out, dx, dsw, part, lpart]), "a guard changed"
    assert not torch.isnan(g_part).any() and not torch.isnan(g_lpart).any(), "a partial slot was left unwritten"
    got = dict(out=g_out, dx=g_dx, dsw=g_dsw, dcw=g_part.double().view(B, nblk // B, 2 * C).sum(1),
               dlc=g_lpart[0].double().sum(), dls=g_lpart[1].double().sum())
    ck = Check("ifrm_combine", rc.ifrm_run_id(run))
    for n in rc.IFRM_OUT:
        if kind == "exact":
            ck.exact(n, got[n], ref[n].to(dt) if n in ("out", "dx", "dsw") else ref[n])
        else:
            ck.within(n, got[n], ref[n], e[n], rc.out_ulp(n, dt), n in rc.ROWWISE)
    ck.done()


def test_refusals(dev):
    buf = Guarded((1 << 16,), F32, dev)
    t, s = buf.t, stream()

    def fwd(B, N, C, dt):
        return try_call("cmx_ifrm_combine_fwd", t, t, t, t, t, t, B, N, C, dt, s)

    def bwd(B, N, C, dt):
        return try_call("cmx_ifrm_combine_bwd", t, t, t, t, t, t, t, t, t, t, B, N, C, dt, s)

    for f in (fwd, bwd):
        assert f(1, 4, 520, 1) == SHAPE and f(1, 4, 516, 0) == SHAPE           # C > 512
        assert f(1, 4, 12, 1) == SHAPE and f(1, 4, 6, 0) == SHAPE              # C % V
        assert f(0, 4, 32, 1) == SHAPE and f(1, 0, 32, 1) == SHAPE and f(1, 4, 0, 2) == SHAPE
    assert try_call("cmx_mul2", t, t, t, 0, s) == SHAPE and try_call("cmx_mul2_bwd", t, t, t, t, t, 0, s) == SHAPE
    assert try_call("cmx_rowln_fwd", t, t, t, t, t, t, 0, 8, 1e-5, s) == SHAPE
    assert try_call("cmx_rowln_fwd", t, t, t, t, t, t, 1, 0, 1e-5, s) == SHAPE
    assert try_call("cmx_rowln_bwd", t, t, t, t, t, t, t, t, 0, 8, s) == SHAPE
    assert try_call("cmx_rowln_bwd", t, t, t, t, t, t, t, t, 1, 0, s) == SHAPE
    torch.cuda.synchronize()
    assert buf.untouched() and buf.intact()
