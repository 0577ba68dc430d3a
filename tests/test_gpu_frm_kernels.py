"""The kernels of csrc/frm.hip through the C-ABI: cmx_frm_combine_fwd / _bwd, cmx_frm_pool_bwd / _fwd and the
channel-MLP GEMV pair cmx_small_linear_fwd / _bwd, at kernel level (h, sw and cw given, not computed).

Cases, fp64 references, the fp32 emulation and the bound 2 E_emul + u: tests/rectify_cases.py (its constructions are
checked on the CPU by tests/test_rectify_cases.py).  Every device buffer is Guarded (tests/kernel_harness.py): NaN
guards on both sides, and every output and partial workspace starts as the NaN pattern and must be NaN-free wherever
a consumer reads it.  Every tensor test launches twice and asks for equal bits.  Exact kinds are torch.equal to the
reference rounded once to the output type; Gaussian kinds print `err bound ratio` before they assert."""
import os
import sys

import pytest
import torch

from rgbx_semantic_segmentation_amd import _lib
from rgbx_semantic_segmentation_amd._lib import call, ptr, query, stream, try_call

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rectify_cases as rc  # noqa: E402
from kernel_harness import CODE, Check, Guarded, all_intact, bits_equal, put, twice  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = torch.float32
SHAPE = _lib.CMX_ERR_SHAPE


# ================================================================================= combine
FWD_RUNS = rc.FRM_RUNS + [(c, "pos") for c in rc.FRM_POS]


@pytest.mark.parametrize("case,kind", FWD_RUNS, ids=[rc.frm_run_id(r) for r in FWD_RUNS])
def test_combine_fwd(dev, case, kind):
    inp = rc.frm_inputs(case, kind)
    ref, e = rc.frm_expected(case, kind)
    B, N, C, dt = case.B, case.N, case.C, case.dtype
    x, h = put(inp["x"], dt, dev), put(inp["h"], dt, dev)
    cw, w2, b2 = put(inp["cw"], F32, dev), put(inp["w2"], F32, dev), put(inp["b2"], F32, dev)
    sw, out = Guarded((B, N, 2), F32, dev), Guarded((2, B, N, C), dt, dev)
    g_sw, g_out = twice(lambda: call("cmx_frm_combine_fwd", x.t, cw.t, h.t, w2.t, b2.t, sw.t, out.t, B, N, C, CODE[dt],
                                     stream()), [sw, out])
    assert all_intact([x, h, cw, w2, b2, sw, out]), "a guard changed"
    ck = Check("combine_fwd", rc.frm_run_id((case, kind)))
    if kind == "gauss":
        ck.within("sw", g_sw, ref["sw"], e["sw"], rc.ULP32, True)
        ck.within("out", g_out, ref["out"], e["out"], rc.ULP[dt], True)
    else:
        assert bits_equal(g_sw, torch.full_like(g_sw, 0.5))
        ck.exact("sw", g_sw, ref["sw"])
        ck.exact("out", g_out, ref["out"].to(dt))
    ck.done()


def run_combine_bwd(dev, case, inp, hb, dout, dout2=None):
    """-> (dx, dh, pcw (B, nblk, 2C), psp (B nblk, 2C + 2)) on the host, launched twice"""
    B, N, C, dt = case.B, case.N, case.C, case.dtype
    nblk = query("cmx_frm_combine_bwd_nblk", N, C, CODE[dt])
    assert nblk == rc.combine_nblk(N, C, case.V) == case.nblk                  # the restatement has not drifted
    nws = query("cmx_frm_combine_bwd_workspace", B, N, C, CODE[dt]) // 4
    assert nws == B * nblk * 2 * C + B * nblk * (2 * C + 2)
    x, h = put(inp["x"], dt, dev), put(hb, dt, dev)
    d, d2 = put(dout, dt, dev), (put(dout2, dt, dev) if dout2 is not None else None)
    cw, w2, sw = put(inp["cw"], F32, dev), put(inp["w2"], F32, dev), put(inp["sw"], F32, dev)
    dx, dh, ws = Guarded((2, B, N, C), dt, dev), Guarded((B, N, C), dt, dev), Guarded((nws,), F32, dev)
    g_dx, g_dh, g_ws = twice(lambda: call("cmx_frm_combine_bwd", d.t, d2.t if d2 else 0, x.t, cw.t, sw.t, h.t, w2.t,
                                          dx.t, dh.t, ws.t, B, N, C, CODE[dt], stream()), [dx, dh, ws])
    assert all_intact([x, h, d, d2, cw, w2, sw, dx, dh, ws]), "a guard changed"
    assert not torch.isnan(g_ws).any(), "a partial slot was left unwritten"
    k = B * nblk * 2 * C
    return g_dx, g_dh, g_ws[:k].view(B, nblk, 2 * C), g_ws[k:].view(B * nblk, 2 * C + 2)


@pytest.mark.parametrize("case,kind", rc.FRM_BWD_RUNS, ids=[rc.frm_run_id(r) for r in rc.FRM_BWD_RUNS])
def test_combine_bwd(dev, case, kind):
    inp = rc.frm_inputs(case, kind)
    ref, e = rc.frm_expected(case, kind)
    C, dt = case.C, case.dtype
    g_dx, g_dh, pcw, psp = run_combine_bwd(dev, case, inp, rc.frm_bwd_h(case, kind), inp["dout"])
    sp = psp.double().sum(0)
    got = dict(dx=g_dx, dh=g_dh, dcw=pcw.double().sum(1), dw2=sp[:2 * C].view(2, C), db2=sp[2 * C:])
    ck = Check("combine_bwd", rc.frm_run_id((case, kind)))
    for n in rc.FRM_BWD_OUT:
        if kind == "gauss":
            ck.within(n, got[n], ref[n], e[n], rc.out_ulp(n, dt), n in rc.ROWWISE)
        else:
            ck.exact(n, got[n], ref[n].to(dt) if n in ("dx", "dh") else ref[n])
    if kind != "gauss":
        z = rc.frm_bwd_h(case, kind) == 0
        assert not g_dh[z].any()                                               # dh == 0 at h == +0.0 and -0.0
    ck.done()


DOUT2 = [(dt, C) for dt in rc.DTYPES for C in (rc.vec_width(dt), 160, 768 if dt != F32 else 320)]


@pytest.mark.parametrize("dtype,C", DOUT2)
def test_combine_bwd_dout2_is_rounded_once(dev, dtype, C):
    """dout2 given == dout2 = NULL on (dout + dout2).to(T) formed on the host in T, bit for bit, on sums that are
    not representable in T (256 + 1 in bf16, 2048 + 1 in fp16) and on ties"""
    case = rc.FrmCase(f"dout2_{rc.name_of(dtype)}_C{C}", dtype, C, 2, rc.rpb_of(C, rc.vec_width(dtype)) + 1, "dout2")
    inp = rc.frm_inputs(case, "gauss")
    d, d2, s = rc.dout2_tensors(dtype, (2, case.B, case.N, C), rc.gen(case.name))
    two = run_combine_bwd(dev, case, inp, inp["h"], d, d2)
    one = run_combine_bwd(dev, case, inp, inp["h"], s)
    for name, a, b in zip(("dx", "dh", "pcw", "psp"), two, one):
        same = bits_equal(a, b)
        rc.report("combine_bwd_dout2", case.name, name, exact=same)
        assert same, name
    if dtype != F32:                               # and the sum carried unrounded would have shown
        assert (s.double() != d.double() + d2.double()).any()


@pytest.mark.parametrize("exact", [True, False], ids=["ints", "gauss"])
@pytest.mark.parametrize("name", ["bfloat16_C160_B3_N67", "float32_C64_B3_N67", "float16_C768_B3_N67"])
def test_dcw_partials_feed_the_gemv_backward(dev, name, exact):
    """the combine backward's dcw partials as cmx_small_linear_bwd's dy, both ways FRMF.backward does it: the slabs
    read in place (nsl = nblk, ss = 2C, sm = nblk 2C) and pre-summed by cmx_partials_sum"""
    case = next(c for c in rc.FRM_CASES if c.name == name)
    kind = "exact" if exact else "gauss"
    inp = rc.frm_inputs(case, kind)
    B, C, nblk, H = case.B, case.C, case.nblk, 24
    _, _, pcw, _ = run_combine_bwd(dev, case, inp, rc.frm_bwd_h(case, kind), inp["dout"])
    g = rc.gen("dcw", name, kind)
    if exact:
        y, x, w = rc.pick(g, (0.5,), B, 2 * C), rc.ints(g, -2, 2, B, H), rc.ints(g, -2, 2, 2 * C, H)
    else:
        y = torch.sigmoid(rc.randn(g, B, 2 * C)).float().double()
        x, w = rc.randn(g, B, H).float().double(), (rc.randn(g, 2 * C, H) / H ** 0.5).float().double()
    part64 = pcw.double().transpose(0, 1).contiguous()                          # (nblk, B, 2C)
    ref = rc.linear_bwd(part64, y, x, w, "sigmoid")[1:]
    e = [0.0, 0.0, 0.0]
    for order in rc.ORDERS:
        emu = rc.linear_bwd(part64.float(), y.float(), x.float(), w.float(), "sigmoid", order)[1:]
        e = [max(a, rc.tenerr(v, r)) for a, v, r in zip(e, emu, ref)]
    slabs = put(pcw.double(), F32, dev)
    yd, xd, wd = put(y, F32, dev), put(x, F32, dev), put(w, F32, dev)
    summed = Guarded((B, 2 * C), F32, dev)
    call("cmx_partials_sum", slabs.t, summed.t, B, nblk, 2 * C, 0, 1.0, stream())
    ck = Check("dcw_to_gemv", f"{name}-{kind}")
    for tag, src, nsl, ss, sm in (("slabs", slabs, nblk, 2 * C, nblk * 2 * C), ("summed", summed, 1, 0, 2 * C)):
        dxp, dw, db = Guarded((rc.NSLICE, B, H), F32, dev), Guarded((2 * C, H), F32, dev), Guarded((2 * C,), F32, dev)
        call("cmx_small_linear_bwd", src.t, nsl, ss, sm, yd.t, xd.t, wd.t, dxp.t, dw.t, db.t, B, H, 2 * C, rc.ACT["sigmoid"],
             0, stream())
        torch.cuda.synchronize()
        assert all_intact([slabs, summed, yd, xd, wd, dxp, dw, db])
        got = (dxp.t.cpu().double().sum(0), dw.t.cpu(), db.t.cpu())
        for n, v, r, ee in zip(("dx", "dw", "db"), got, ref, e):
            if exact:
                ck.exact(f"{tag} {n}", v, r)
            else:
                ck.within(f"{tag} {n}", v, r, ee, rc.ULP32, False)
    ck.done()


# ================================================================================= pooling
@pytest.mark.parametrize("case", rc.POOL_BWD_CASES, ids=lambda c: c.name)
def test_pool_bwd(dev, case):
    part, am, dx0 = rc.pool_bwd_inputs(case)
    ref, e = rc.pool_bwd_expected(case)
    B, N, C, dt, ns = case.B, case.N, case.C, case.dtype, case.nslice
    stride = B * 4 * C + 24                        # the padding between the slices stays NaN: it is never read
    pbuf = Guarded((ns, stride), F32, dev)
    pbuf.t[:, :B * 4 * C] = part.view(ns, -1).float().to(dev)
    amd = Guarded((B, 2 * C), torch.int32, dev, am)
    dx = Guarded((2, B, N, C), dt, dev, dx0.to(dt))
    (got,) = twice(lambda: call("cmx_frm_pool_bwd", pbuf.t, ns, stride, amd.t, dx.t, B, N, C, CODE[dt], stream()), [dx],
                   prefill=lambda: dx.t.copy_(dx0.to(dt)))
    assert all_intact([pbuf, amd, dx]), "a guard changed"
    ck = Check("pool_bwd", case.name)
    if case.kind == "exact":
        ck.exact("dx", got, ref)
    else:
        ck.within("dx", got, ref, e, rc.ULP[dt], True)
    ck.done()


POOL_FWD = [(torch.float16, 1024, 2, 77), (torch.float16, 32, 1, 1), (torch.float16, 160 * 2, 3, 300),
            (torch.bfloat16, 1024, 3, 300), (F32, 1024, 1, 50)]


@pytest.mark.parametrize("dtype,C,B,N", POOL_FWD)
def test_pool_fwd_guarded(dev, dtype, C, B, N):
    """avg against fp64 (2 E_emul + u), max exact, argmax the first maximal token (values quantised so ties occur);
    pooled, argmax and the workspace between guards, the tickets back at zero"""
    g = rc.gen("poolfwd", dtype, C, B, N)
    x = (rc.randn(g, 2, B, N, C) * 4).round()
    xd = put(x, dtype, dev)
    pooled, argmax = Guarded((B, 4 * C), F32, dev), Guarded((B, 2 * C), torch.int32, dev)
    ws = Guarded((query("cmx_frm_pool_workspace", B, N, C) // 4,), F32, dev)
    ntk = query("cmx_frm_pool_tickets", B, C)
    tk = Guarded((ntk,), torch.int32, dev, torch.zeros(ntk, dtype=torch.int32))
    g_pooled, g_arg = twice(lambda: call("cmx_frm_pool_fwd", xd.t, pooled.t, argmax.t, ws.t, tk.t, B, N, C, CODE[dtype],
                                         stream()), [pooled, argmax])
    assert all_intact([xd, pooled, argmax, ws, tk]) and not bool(tk.t.any())
    xf = x.permute(1, 0, 3, 2).reshape(B, 2 * C, N)
    avg, mx = xf.mean(-1), xf.amax(-1)
    first = (xf == mx[..., None]).float().argmax(-1).to(torch.int32)
    e = max(rc.tenerr(rc._sum(xf.float(), -1, o) / N, avg) for o in rc.ORDERS)
    ck = Check("pool_fwd", f"{rc.name_of(dtype)}_C{C}_B{B}_N{N}")
    ck.within("avg", g_pooled[:, :2 * C], avg, e, rc.ULP32, False)
    ck.exact("max", g_pooled[:, 2 * C:], mx)
    ck.exact("argmax", g_arg, first)
    ck.done()


# ================================================================================= the GEMV pair
@pytest.mark.parametrize("case", rc.LIN_FWD_CASES, ids=lambda c: c.name)
def test_small_linear_fwd(dev, case):
    x, w, b = rc.lin_fwd_inputs(case)
    ref, e = rc.lin_fwd_expected(case)
    M, K, Nout = case.M, case.K, case.Nout
    xd, wd, bd = put(x, F32, dev), put(w, F32, dev), (put(b, F32, dev) if b is not None else None)
    y = Guarded((M, Nout), F32, dev)
    (got,) = twice(lambda: call("cmx_small_linear_fwd", xd.t, wd.t, bd.t if bd else 0, y.t, M, K, Nout, rc.ACT[case.act],
                                stream()), [y])
    assert all_intact([xd, wd, bd, y]), "a guard changed"
    ck = Check("small_linear_fwd", case.name)
    if case.kind == "exact":
        ck.exact("y", got, ref)
    else:
        ck.within("y", got, ref, e, rc.ULP32, False)
    ck.done()


@pytest.mark.parametrize("case", rc.LIN_BWD_CASES, ids=lambda c: c.name)
def test_small_linear_bwd(dev, case):
    part, y, x, w, dw0, db0 = rc.lin_bwd_inputs(case)
    ref, e = rc.lin_bwd_expected(case)
    M, K, Nout, ns, acc = case.M, case.K, case.Nout, case.nslice, case.accumulate
    pd, yd, xd, wd = put(part, F32, dev), put(y, F32, dev), put(x, F32, dev), put(w, F32, dev)
    dxp = Guarded((rc.NSLICE, M, K), F32, dev) if case.dxp else None
    dw = Guarded((Nout, K), F32, dev)
    db = Guarded((Nout,), F32, dev) if case.db else None

    def prefill():
        if acc:
            dw.t.copy_(dw0.float())
            if db:
                db.t.copy_(db0.float())

    prefill()
    ss = 0 if ns == 1 else M * Nout
    outs = [o for o in (dxp, dw, db) if o is not None]
    got = twice(lambda: call("cmx_small_linear_bwd", pd.t, ns, ss, Nout, yd.t, xd.t, wd.t, dxp.t if dxp else 0, dw.t,
                             db.t if db else 0, M, K, Nout, rc.ACT[case.act], acc, stream()), outs, prefill=prefill)
    assert all_intact([pd, yd, xd, wd, dxp, dw, db]), "a guard changed"
    got = dict(zip([n for n, o in zip(("dx", "dw", "db"), (dxp, dw, db)) if o is not None], got))
    ck = Check("small_linear_bwd", case.name)
    if "dx" in got:
        assert not torch.isnan(got["dx"]).any(), "a dx_part slice was left unwritten"
        per = -(-Nout // rc.NSLICE)
        empty = [s for s in range(rc.NSLICE) if s * per >= Nout]
        assert (len(empty) == 6) == (Nout == 10)
        for s in empty:                            # an empty slice is written, as zeros
            assert not got["dx"][s].any(), s
        got["dx"] = got["dx"].double().sum(0)
    for i, n in enumerate(("dx", "dw", "db")):
        if n in got:
            if case.kind == "exact":
                ck.exact(n, got[n], ref[i])
            else:
                ck.within(n, got[n], ref[i], e[i], rc.ULP32, False)
    ck.done()


# ================================================================================= refusals
def test_refusals(dev):
    """one argument over its limit each: CMX_ERR_SHAPE from the host-side check, before any launch; the buffer
    every pointer argument names still holds its fill pattern afterwards"""
    buf = Guarded((1 << 16,), F32, dev)
    t, s = buf.t, stream()
    p = ptr(t)
    tk = Guarded((8192,), torch.int32, dev)

    def fwd(B, N, C, dt):
        return try_call("cmx_frm_combine_fwd", t, t, t, t, t, t, t, B, N, C, dt, s)

    def bwd(B, N, C, dt):
        return try_call("cmx_frm_combine_bwd", t, 0, t, t, t, t, t, t, t, t, B, N, C, dt, s)

    for f in (fwd, bwd):
        assert f(1, 4, 12, 1) == SHAPE and f(1, 4, 6, 0) == SHAPE                  # C % V
        assert f(1, 4, 1032, 1) == SHAPE and f(1, 4, 516, 0) == SHAPE              # C / V > 128
        assert f(0, 4, 32, 1) == SHAPE and f(1, 0, 32, 1) == SHAPE and f(1, 4, 0, 1) == SHAPE
        assert f(-1, 4, 32, 0) == SHAPE and f(1, -4, 32, 2) == SHAPE

    def pool(ns, B, N, C, dt):
        return try_call("cmx_frm_pool_bwd", t, ns, 4 * C * max(B, 1), tk.t, t, B, N, C, dt, s)

    assert pool(17, 1, 4, 32, 1) == SHAPE and pool(0, 1, 4, 32, 1) == SHAPE        # nslice
    assert pool(1, 1, 4, 1028, 1) == SHAPE and pool(1, 1, 4, 1028, 0) == SHAPE     # C = 1028
    assert pool(1, 1, 4, 1032, 2) == SHAPE and pool(1, 1, 4, 12, 1) == SHAPE
    assert pool(1, 0, 4, 32, 1) == SHAPE and pool(1, 1, 0, 32, 1) == SHAPE and pool(1, 1, 4, 0, 0) == SHAPE

    def lf(M, K, Nout, xo=0, wo=0):
        return try_call("cmx_small_linear_fwd", p + xo, p + wo, 0, t, M, K, Nout, 0, s)

    assert lf(9, 4, 4) == SHAPE and lf(0, 4, 4) == SHAPE                            # M
    assert lf(1, 6, 4) == SHAPE and lf(1, 0, 4) == SHAPE and lf(1, -4, 4) == SHAPE  # K
    assert lf(8, 2052, 4) == SHAPE and lf(5, 3280, 4) == SHAPE                      # M K 4 > 64 KiB
    assert lf(1, 4, 4, xo=4) == SHAPE and lf(1, 4, 4, wo=8) == SHAPE                # alignment
    assert lf(1, 4, 0) == SHAPE

    def lb(ns, M, K, Nout):
        return try_call("cmx_small_linear_bwd", t, ns, 0, Nout, t, t, t, t, t, t, M, K, Nout, 0, 0, s)

    assert lb(1, 9, 4, 4) == SHAPE and lb(1, 0, 4, 4) == SHAPE and lb(0, 1, 4, 4) == SHAPE
    assert lb(1, 1, 4, 4097) == SHAPE and lb(1, 1, 0, 4) == SHAPE and lb(1, 1, 4, 0) == SHAPE

    def pf(B, N, C):
        return try_call("cmx_frm_pool_fwd", t, t, tk.t, t, tk.t, B, N, C, 1, s)

    assert pf(65, 4, 1024) == SHAPE                                                 # too many tickets: 2 B C / 32 > 4096
    assert pf(1, 4, 48) == SHAPE and pf(1, 0, 32) == SHAPE and pf(0, 4, 32) == SHAPE
    torch.cuda.synchronize()
    assert buf.untouched() and tk.untouched() and buf.intact() and tk.intact()
