"""Every instantiation of the LayerNorm kernels (csrc/layernorm.hip; the launch policy is csrc/ln_plan.h)
against fp64 references (tests/norm_cases.py: the case table, the input kinds, the references and the
emulated yardstick; tests/test_norm_cases.py checks the constructions and the plans on the CPU).

For every case, every dtype the case lists, both of the model's eps values and every input kind:
  forward      y per row, mean and rstd per tensor within 2 E_emul + u; const rows give y == beta rounded to
               the storage type and mean == the constant bit for bit.
  backward     cmx_layernorm_bwd: dx per row, dgamma and dbeta within the bound, dbeta == the integer column
               sum exactly; cmx_layernorm_bwd_res with every optional operand NULL is bit-identical to it.
  bwd_res      dy2, dres and dxs + sscale each alone and all together against fp64; dxs == sscale dx on the
               stored tensors wherever the sample's scale is 0 or a power of two.
  accumulate   pre-filled dgamma / dbeta: accumulate = 1 is bit-identical to pre-fill + the accumulate = 0 result.
  NULL mode    dgamma = dbeta = NULL (the deferred mode): dx bit-identical, the workspace (G, nb, 2C) with
               nb = bytes / (8 G C) sums over nb to dgamma within the bound and to dbeta exactly.
  containment  one case per plan: every output and the workspace (sized exactly as queried) inside a larger
               buffer of sentinels; bit-identical to the packed run, sentinels untouched on both sides.
  refusals     C no multiple of the vector width, C > 1024, dxs without sscale raise before any launch;
               R = 0 forward returns OK and writes nothing.
Every figure is printed before it is asserted ([norm] lines)."""
import os
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import norm_cases as nc  # noqa: E402

pytestmark = pytest.mark.gpu

RUNS = nc.ln_runs()
IDS = [nc.ln_run_id(r) for r in RUNS]


def on_dev(inp, dtype, dev):
    return SimpleNamespace(x=inp.x.to(dev, dtype), gamma=inp.gamma.float().to(dev), beta=inp.beta.float().to(dev),
                           dy=inp.dy.to(dev, dtype), dy2=inp.dy2.to(dev, dtype), dres=inp.dres.to(dev, dtype),
                           sscale=inp.sscale.float().to(dev))


def checker(case, dtype, eps, kind, exp):
    return nc.Checker("ln", f"{case.name} {nc.name_of(dtype)} eps={eps:g} {kind}", exp, dtype)


def forward(K, d, case, eps):
    y, mean, rstd = K.layernorm_fwd(d.x, d.gamma, d.beta, eps, G=case.G)
    return y, mean, rstd


def grads(case, dev, fill=None):
    if fill is None:
        return torch.empty(case.G, case.C, device=dev), torch.empty(case.G, case.C, device=dev)
    g = torch.Generator().manual_seed(5)
    return tuple(torch.randint(-9, 10, (case.G, case.C), generator=g).float().to(dev) for _ in range(2))


def bwd_res(K, d, case, mean, rstd, variant, dgamma, dbeta, accumulate=False):
    two, res, sc = nc._uses(variant)
    dxs = torch.empty_like(d.x) if sc else None
    dx, part = K.layernorm_bwd_res(d.dy, d.x, d.gamma, mean, rstd, case.G, dgamma, dbeta, dy2=d.dy2 if two else None,
                                   dres=d.dres if res else None, sscale=d.sscale if sc else None,
                                   rows_per_sample=case.rps, dxs=dxs, accumulate=accumulate)
    return dx, dxs, part


@pytest.mark.parametrize("run", RUNS, ids=IDS)
def test_ln_forward(dev, run):
    from rgbx_semantic_segmentation_amd import kernels as K
    case, dtype, eps = run
    done = []
    for kind in case.kinds:
        exp = nc.ln_expected(case, kind, dtype, eps)
        ck = checker(case, dtype, eps, kind, exp)
        y, mean, rstd = forward(K, on_dev(exp.inp, dtype, dev), case, eps)
        assert torch.isfinite(y).all() and torch.isfinite(mean).all() and torch.isfinite(rstd).all()
        ck.within("fwd", "y", y, exp.ref.y)
        ck.within("fwd", "mean", mean, exp.ref.mean)
        ck.within("fwd", "rstd", rstd, exp.ref.rstd)
        if kind == "const":
            beta = exp.inp.beta.to(dtype).double()[:, None, :].expand(case.G, case.R, case.C).reshape(-1, case.C)
            ck.exact("fwd const y == beta", y, beta)
            ck.exact("fwd const mean", mean, exp.inp.x[:, 0])
        done.append(ck)
    nc.finish(done)


@pytest.mark.parametrize("run", RUNS, ids=IDS)
def test_ln_backward(dev, run):
    from rgbx_semantic_segmentation_amd import kernels as K
    case, dtype, eps = run
    done = []
    for kind in case.kinds:
        exp = nc.ln_expected(case, kind, dtype, eps)
        ck = checker(case, dtype, eps, kind, exp)
        d = on_dev(exp.inp, dtype, dev)
        _, mean, rstd = forward(K, d, case, eps)
        dg, db = grads(case, dev)
        dx = K.layernorm_bwd(d.dy, d.x, d.gamma, mean, rstd, case.G, dg, db)
        want = nc.ln_expected_bwd(case, exp.inp, exp.ref, "plain")
        ck.within("bwd", ("plain", "dx"), dx, want.dx)
        ck.within("bwd", ("plain", "dgamma"), dg, want.dgamma)
        ck.within("bwd", ("plain", "dbeta"), db, want.dbeta)
        ck.exact("bwd dbeta == integer column sum", db, exp.inp.dy.view(case.G, case.R, case.C).sum(1))
        dg2, db2 = grads(case, dev)
        dx2, _, _ = bwd_res(K, d, case, mean, rstd, "plain", dg2, db2)
        for name, a, b in (("dx", dx2, dx), ("dgamma", dg2, dg), ("dbeta", db2, db)):
            ck.exact(f"bwd_res all NULL == bwd {name}", a, b)
        done.append(ck)
    nc.finish(done)


@pytest.mark.parametrize("run", RUNS, ids=IDS)
def test_ln_bwd_res(dev, run):
    from rgbx_semantic_segmentation_amd import kernels as K
    case, dtype, eps = run
    done = []
    for kind in case.kinds:
        exp = nc.ln_expected(case, kind, dtype, eps)
        ck = checker(case, dtype, eps, kind, exp)
        d = on_dev(exp.inp, dtype, dev)
        _, mean, rstd = forward(K, d, case, eps)
        for variant in ("dy2", "dres", "sscale", "all"):
            dg, db = grads(case, dev)
            dx, dxs, _ = bwd_res(K, d, case, mean, rstd, variant, dg, db)
            want = nc.ln_expected_bwd(case, exp.inp, exp.ref, variant)
            ck.within(variant, (variant, "dx"), dx, want.dx)
            ck.within(variant, (variant, "dgamma"), dg, want.dgamma)
            ck.within(variant, (variant, "dbeta"), db, want.dbeta)
            ck.exact(f"{variant} dbeta == integer column sum", db, want.dbeta)
            if dxs is not None:
                ck.within(variant, (variant, "dxs"), dxs, want.dxs)
                s = exp.inp.sscale[nc.sample_of_row(case)][:, None]
                dxc, dxsc = dx.cpu().double(), dxs.cpu().double()
                pow2 = nc.pow2_exact(s, dxc, dtype)
                ck.exact(f"{variant} dxs == sscale dx at power-of-two scales", dxsc[pow2], (s * dxc)[pow2])
        done.append(ck)
    nc.finish(done)


@pytest.mark.parametrize("run", RUNS, ids=IDS)
def test_ln_accumulate(dev, run):
    from rgbx_semantic_segmentation_amd import kernels as K
    case, dtype, eps = run
    kind = case.kinds[0]
    exp = nc.ln_expected(case, kind, dtype, eps)
    ck = checker(case, dtype, eps, kind, exp)
    d = on_dev(exp.inp, dtype, dev)
    _, mean, rstd = forward(K, d, case, eps)
    for variant in ("plain", "all"):
        dg0, db0 = grads(case, dev)
        dx0, dxs0, _ = bwd_res(K, d, case, mean, rstd, variant, dg0, db0)
        pg, pb = grads(case, dev, fill=True)
        dg1, db1 = pg.clone(), pb.clone()
        dx1, dxs1, _ = bwd_res(K, d, case, mean, rstd, variant, dg1, db1, accumulate=True)
        ck.exact(f"accumulate {variant} dgamma", dg1, pg + dg0)
        ck.exact(f"accumulate {variant} dbeta", db1, pb + db0)
        ck.exact(f"accumulate {variant} dx", dx1, dx0)
        if dxs0 is not None:
            ck.exact(f"accumulate {variant} dxs", dxs1, dxs0)
    dg0, db0 = grads(case, dev)
    K.layernorm_bwd(d.dy, d.x, d.gamma, mean, rstd, case.G, dg0, db0)
    pg, pb = grads(case, dev, fill=True)
    dg1, db1 = pg.clone(), pb.clone()
    K.layernorm_bwd(d.dy, d.x, d.gamma, mean, rstd, case.G, dg1, db1, accumulate=True)
    ck.exact("accumulate cmx_layernorm_bwd dgamma", dg1, pg + dg0)
    ck.exact("accumulate cmx_layernorm_bwd dbeta", db1, pb + db0)
    assert not torch.equal(dg1, dg0) and not torch.equal(db1, db0)          # the pre-fill counted
    nc.finish([ck])


@pytest.mark.parametrize("run", RUNS, ids=IDS)
def test_ln_null_mode(dev, run):
    """dgamma = dbeta = NULL: the per-block partials stay in the workspace for the caller's grouped reduce"""
    from rgbx_semantic_segmentation_amd import kernels as K
    case, dtype, eps = run
    kind = case.kinds[0]
    exp = nc.ln_expected(case, kind, dtype, eps)
    ck = checker(case, dtype, eps, kind, exp)
    d = on_dev(exp.inp, dtype, dev)
    _, mean, rstd = forward(K, d, case, eps)
    nbytes = K.query("cmx_layernorm_bwd_workspace", case.R, case.G, case.C, nc.dtype_code(dtype))
    nb = nbytes // (8 * case.G * case.C)
    assert nb == min(512, -(-case.R // (256 // case.bwd[0]))) and nbytes == case.G * nb * 2 * case.C * 4
    for variant in ("plain", "all"):
        dg, db = grads(case, dev)
        dx0, dxs0, _ = bwd_res(K, d, case, mean, rstd, variant, dg, db)
        dx1, dxs1, part = bwd_res(K, d, case, mean, rstd, variant, None, None)
        assert part.shape == (case.G, nb, 2 * case.C)
        ck.exact(f"NULL {variant} dx", dx1, dx0)
        if dxs0 is not None:
            ck.exact(f"NULL {variant} dxs", dxs1, dxs0)
        tot = part.double().view(case.G, nb, 2, case.C).sum(1).cpu()
        want = nc.ln_expected_bwd(case, exp.inp, exp.ref, variant)
        ck.within(f"NULL {variant}", (variant, "dgamma"), tot[:, 0], want.dgamma)
        ck.exact(f"NULL {variant} partials sum to dbeta", tot[:, 1], want.dbeta)
    nc.finish([ck])


# --------------------------------------------------------------------------------- containment
Guard = nc.Guard
CONTAIN = [(c, dt) for c in nc.LN_CONTAINMENT for dt in c.dtypes]


@pytest.mark.parametrize("run", CONTAIN, ids=[f"{c.name}-{nc.name_of(dt)}" for c, dt in CONTAIN])
def test_ln_containment(dev, run):
    from rgbx_semantic_segmentation_amd import kernels as K
    case, dtype = run
    eps, code = nc.LN_EPS[0], nc.dtype_code(dtype)
    exp = nc.ln_expected(case, case.kinds[0], dtype, eps)
    d = on_dev(exp.inp, dtype, dev)
    rows, G, C, R = case.rows, case.G, case.C, case.R
    # packed
    y0, mean0, rstd0 = forward(K, d, case, eps)
    dg0, db0 = grads(case, dev)
    dx0, dxs0, _ = bwd_res(K, d, case, mean0, rstd0, "all", dg0, db0)
    # guarded, through the C ABI
    y, dx, dxs = (Guard(rows * C, dtype, dev) for _ in range(3))
    mean, rstd = Guard(rows, torch.float32, dev), Guard(rows, torch.float32, dev)
    dg, db = Guard(G * C, torch.float32, dev), Guard(G * C, torch.float32, dev)
    nbytes = K.query("cmx_layernorm_bwd_workspace", R, G, C, code)
    assert nbytes % 16 == 0 or nbytes % 4 == 0
    ws = Guard(nbytes // 4, torch.float32, dev)
    K.call("cmx_layernorm_fwd", K.ptr(d.x), K.ptr(d.gamma), K.ptr(d.beta), y.ptr(), mean.ptr(), rstd.ptr(), R, G, C,
           float(eps), code, K.stream())
    K.call("cmx_layernorm_bwd_res", K.ptr(d.dy), K.ptr(d.dy2), K.ptr(d.x), K.ptr(d.gamma), mean.ptr(), rstd.ptr(),
           K.ptr(d.dres), K.ptr(d.sscale), dxs.ptr(), dx.ptr(), dg.ptr(), db.ptr(), ws.ptr(), R, G, C, case.rps, 0, code,
           K.stream())
    torch.cuda.synchronize()
    guards = dict(y=y, mean=mean, rstd=rstd, dx=dx, dxs=dxs, dgamma=dg, dbeta=db, workspace=ws)
    for name, g in guards.items():
        assert g.intact(), f"{case.name}: a store outside the logical {name}"
    packed = dict(y=y0, mean=mean0, rstd=rstd0, dx=dx0, dxs=dxs0, dgamma=dg0, dbeta=db0)
    for name, t in packed.items():
        assert torch.equal(guards[name].view.view(t.shape), t), (case.name, name)
    # the NULL mode writes the same workspace and nothing else
    ws2, dx2 = Guard(nbytes // 4, torch.float32, dev), Guard(rows * C, dtype, dev)
    K.call("cmx_layernorm_bwd", K.ptr(d.dy), K.ptr(d.x), K.ptr(d.gamma), mean.ptr(), rstd.ptr(), dx2.ptr(), 0, 0,
           ws2.ptr(), R, G, C, 0, code, K.stream())
    torch.cuda.synchronize()
    assert ws2.intact() and dx2.intact() and not (ws2.view == nc.SENTINEL).any()


# ------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("what", ["vector_width", "too_wide", "dxs_without_sscale", "no_rows"])
def test_ln_refusals(dev, dtype, what):
    """refused before any launch (the outputs keep their sentinel); R = 0 forward is OK and writes nothing"""
    from rgbx_semantic_segmentation_amd import kernels as K
    from rgbx_semantic_segmentation_amd._lib import CMXError
    V, code, R, G = nc.vec_width(dtype), nc.dtype_code(dtype), 70, 2
    C = {"vector_width": 64 + V // 2, "too_wide": 1024 + V}.get(what, 64)
    n = G * R * C
    x = torch.ones(n, device=dev, dtype=dtype)
    gamma = torch.ones(G * C, device=dev)
    stat = torch.ones(G * R, device=dev)
    sent = lambda m, dt: torch.full((m,), nc.SENTINEL, device=dev, dtype=dt)  # noqa: E731
    y, dx, dxs = sent(n, dtype), sent(n, dtype), sent(n, dtype)
    mean, rstd, dg, db = sent(G * R, torch.float32), sent(G * R, torch.float32), sent(G * C, torch.float32), \
        sent(G * C, torch.float32)
    ws = sent(max(1, K.query("cmx_layernorm_bwd_workspace", R, G, 1024, code) // 4), torch.float32)
    p = K.ptr
    if what == "no_rows":
        K.call("cmx_layernorm_fwd", p(x), p(gamma), p(gamma), p(y), p(mean), p(rstd), 0, G, C, 1e-6, code, K.stream())
    elif what == "dxs_without_sscale":
        with pytest.raises(CMXError):
            K.call("cmx_layernorm_bwd_res", p(x), 0, p(x), p(gamma), p(stat), p(stat), 0, 0, p(dxs), p(dx), p(dg), p(db),
                   p(ws), R, G, C, 37, 0, code, K.stream())
    else:
        with pytest.raises(CMXError):
            K.call("cmx_layernorm_fwd", p(x), p(gamma), p(gamma), p(y), p(mean), p(rstd), R, G, C, 1e-6, code, K.stream())
        with pytest.raises(CMXError):
            K.call("cmx_layernorm_bwd", p(x), p(x), p(gamma), p(stat), p(stat), p(dx), p(dg), p(db), p(ws), R, G, C, 0,
                   code, K.stream())
        with pytest.raises(CMXError):
            K.call("cmx_layernorm_bwd_res", p(x), 0, p(x), p(gamma), p(stat), p(stat), 0, p(stat), p(dxs), p(dx), p(dg),
                   p(db), p(ws), R, G, C, 37, 0, code, K.stream())
    torch.cuda.synchronize()
    for t in (y, dx, dxs, mean, rstd, dg, db, ws):
        assert (t == nc.SENTINEL).all()
