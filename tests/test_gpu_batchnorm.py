"""The BatchNorm kernels (csrc/batchnorm.hip), multi-launch and one-launch small path, against fp64 references
(tests/norm_cases.py: the case table, the input kinds, the references and the emulated yardstick;
tests/test_norm_cases.py checks the constructions on the CPU).

For every case, every dtype it lists, eps 1e-5 and 1e-3 and every input kind:
  values       y, dx, dres per channel; mean, invstd, dgamma, dbeta and the running statistics per tensor, within
               2 E_emul + u; the fp64 sums to 1e-12; a constant channel gives mean == the constant and
               invstd == (float) eps^-1/2 bit for bit (the 0.1 channel: within one fp32 unit); dbeta == the integer
               column sum with act = none.  nblk = cmx_bn_workspace / (16 C) is what the case is meant for.
  eval         cmx_bn_finalize(training = 0), the apply and cmx_bn_bwd_apply(training = 0).
  SyncBN       two shards on one GPU: cmx_bn_stats per shard, summed fp64 sums, cmx_bn_finalize(count = M), apply per
               shard; cmx_bn_bwd_reduce per shard, summed sums, cmx_bn_bwd_apply(count = M) per shard: the fp64
               reference of the unsplit batch; dgamma / dbeta are the per-shard local sums.
  accumulate   cmx_bn_bwd_reduce and cmx_bn_small_bwd: bit-identical to pre-fill + overwrite.
  small/multi  the same mean, invstd and sums to fp64 rounding, y / dx within the bound of one another.
  containment  every output and the workspace (exactly cmx_bn_workspace) inside sentinels; bit-identical to the
               packed run.
Every figure is printed before it is asserted ([norm] lines)."""
import os
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import norm_cases as nc  # noqa: E402

pytestmark = pytest.mark.gpu

RUNS = nc.bn_runs()
ACT = {"none": 0, "relu": 2}
F64 = torch.float64


def run_id(r):
    c, dt, eps = r
    return f"{c.name}-{nc.name_of(dt)}-eps{eps:g}"


IDS = [run_id(r) for r in RUNS]


def on_dev(inp, dtype, dev):
    opt = lambda t, dt: None if t is None else t.to(dev, dt)  # noqa: E731
    return SimpleNamespace(x=inp.x.to(dev, dtype), gamma=inp.gamma.float().to(dev), beta=inp.beta.float().to(dev),
                           res=opt(inp.res, dtype), dscale=opt(inp.dscale, torch.float32), dy=inp.dy.to(dev, dtype),
                           rm0=inp.rm0.float().to(dev), rv0=inp.rv0.float().to(dev))


def Checker(case, dtype, eps, kind, exp, mode):
    return nc.Checker("bn", f"{case.name} {nc.name_of(dtype)} eps={eps:g} {kind} {mode}", exp, dtype)


def f32(n, dev):
    return torch.empty(n, dtype=torch.float32, device=dev)


def bn_ws(K, M, C, dev):
    return torch.empty(max(1, K.query("cmx_bn_workspace", M, C) // 8), dtype=F64, device=dev)


def dscale_of(d, row0, case):
    return None if d.dscale is None else d.dscale[row0 // case.rps:]


def apply_fwd(K, x, res, dscale, d, mean, invstd, case, code):
    y = torch.empty_like(x)
    K.call("cmx_bn_apply", K.ptr(x), K.ptr(mean), K.ptr(invstd), K.ptr(d.gamma), K.ptr(d.beta), K.ptr(res), K.ptr(dscale),
           K.ptr(y), x.shape[0], case.C, case.rps, ACT[case.act], code, K.stream())
    return y


def multi_fwd(K, d, case, eps, dtype, training=True):
    M, C, dev, code = case.M, case.C, d.x.device, nc.dtype_code(dtype)
    mean, invstd, rm, rv = f32(C, dev), f32(C, dev), d.rm0.clone(), d.rv0.clone()
    sums = None
    if training:
        sums = torch.empty(2, C, dtype=F64, device=dev)
        K.call("cmx_bn_stats_finalize", K.ptr(d.x), K.ptr(sums), K.ptr(bn_ws(K, M, C, dev)), M, C, float(eps),
               case.momentum, K.ptr(rm), K.ptr(rv), K.ptr(mean), K.ptr(invstd), code, K.stream())
    else:
        K.call("cmx_bn_finalize", 0, 1.0, float(eps), case.momentum, K.ptr(rm), K.ptr(rv), K.ptr(mean), K.ptr(invstd), C,
               0, K.stream())
    y = apply_fwd(K, d.x, d.res, d.dscale, d, mean, invstd, case, code)
    return SimpleNamespace(y=y, mean=mean, invstd=invstd, rmean=rm, rvar=rv, sums=sums)


def bwd_reduce(K, dy, x, res, dscale, d, mean, invstd, case, code, dgamma, dbeta, accumulate=0):
    M, C = x.shape
    sums = torch.empty(2, C, dtype=F64, device=x.device)
    K.call("cmx_bn_bwd_reduce", K.ptr(dy), K.ptr(x), K.ptr(mean), K.ptr(invstd), K.ptr(d.gamma), K.ptr(d.beta),
           K.ptr(res), K.ptr(dscale), K.ptr(sums), K.ptr(dgamma), K.ptr(dbeta), K.ptr(bn_ws(K, M, C, x.device)), M, C,
           case.rps, ACT[case.act], int(accumulate), code, K.stream())
    return sums


def bwd_apply(K, dy, x, res, dscale, d, mean, invstd, sums, count, case, code, training=True):
    dx = torch.empty_like(x)
    dres = torch.empty_like(x) if res is not None else None
    K.call("cmx_bn_bwd_apply", K.ptr(dy), K.ptr(x), K.ptr(mean), K.ptr(invstd), K.ptr(d.gamma), K.ptr(d.beta),
           K.ptr(res), K.ptr(dscale), K.ptr(sums), float(count), K.ptr(dx), K.ptr(dres), x.shape[0], case.C, case.rps,
           ACT[case.act], int(training), code, K.stream())
    return dx, dres


def multi_bwd(K, d, case, f, dtype, training=True):
    code, dev = nc.dtype_code(dtype), d.x.device
    dg, db = f32(case.C, dev), f32(case.C, dev)
    sums = bwd_reduce(K, d.dy, d.x, d.res, d.dscale, d, f.mean, f.invstd, case, code, dg, db)
    dx, dres = bwd_apply(K, d.dy, d.x, d.res, d.dscale, d, f.mean, f.invstd, sums, case.M, case, code, training)
    return SimpleNamespace(dx=dx, dres=dres, dgamma=dg, dbeta=db, sums=sums)


def small_fwd(K, d, case, eps, dtype):
    M, C, dev = case.M, case.C, d.x.device
    mean, invstd, rm, rv = f32(C, dev), f32(C, dev), d.rm0.clone(), d.rv0.clone()
    sums, y = torch.empty(2, C, dtype=F64, device=dev), torch.empty_like(d.x)
    K.call("cmx_bn_small_fwd", K.ptr(d.x), K.ptr(d.res), K.ptr(d.gamma), K.ptr(d.beta), K.ptr(d.dscale), K.ptr(y),
           K.ptr(sums), K.ptr(mean), K.ptr(invstd), K.ptr(rm), K.ptr(rv), M, C, case.rps, ACT[case.act], float(eps),
           case.momentum, nc.dtype_code(dtype), K.stream())
    return SimpleNamespace(y=y, mean=mean, invstd=invstd, rmean=rm, rvar=rv, sums=sums)


def small_bwd(K, d, case, f, dtype, dg=None, db=None, accumulate=0):
    dev = d.x.device
    dg = f32(case.C, dev) if dg is None else dg
    db = f32(case.C, dev) if db is None else db
    dx = torch.empty_like(d.x)
    dres = torch.empty_like(d.x) if d.res is not None else None
    K.call("cmx_bn_small_bwd", K.ptr(d.dy), K.ptr(d.x), K.ptr(f.mean), K.ptr(f.invstd), K.ptr(d.gamma), K.ptr(d.beta),
           K.ptr(d.res), K.ptr(d.dscale), K.ptr(dg), K.ptr(db), K.ptr(dx), K.ptr(dres), case.M, case.C, case.rps,
           ACT[case.act], int(accumulate), nc.dtype_code(dtype), K.stream())
    return SimpleNamespace(dx=dx, dres=dres, dgamma=dg, dbeta=db)


def check_fwd(ck, f, exp, case, kind, eps, training=True):
    ref, inp = exp.ref, exp.inp
    for n in ("y", "mean", "invstd", "rmean", "rvar"):
        assert torch.isfinite(getattr(f, n)).all(), (ck.tag, n)
        ck.within("fwd", n, getattr(f, n), getattr(ref, n))
    if not training:
        return
    ck.close64("sum x", f.sums[0], inp.x.sum(0), inp.x.abs().sum(0))
    ck.close64("sum x^2", f.sums[1], (inp.x ** 2).sum(0), (inp.x ** 2).sum(0))
    if kind == "const":
        dyadic = torch.ones(case.C, dtype=torch.bool)
        dyadic[1:2] = False
        want = nc.f32_invstd_of_zero_variance(eps)
        ck.exact("const mean", f.mean.cpu()[dyadic], inp.x[0][dyadic])
        ck.exact("const invstd == (float) eps^-1/2", f.invstd.cpu()[dyadic], torch.full((int(dyadic.sum()),), want))
        if case.C > 1:          # the 0.1 channel: E[x^2] - mean^2 is fp64 noise of either sign beside eps
            ck.exact("0.1 channel mean", f.mean.cpu()[1], inp.x[0, 1].float())
            off = abs(f.invstd.cpu()[1].item() - want) / want
            print(f"[norm] bn {ck.tag} | 0.1 channel invstd off by {off:.3e}")
            if not off <= 2.0 ** -23:
                ck.bad.append(("clamped variance", off))


def check_bwd(ck, b, exp, case):
    ref = exp.ref
    for n in ("dx", "dres", "dgamma", "dbeta"):
        if getattr(ref, n) is not None:
            assert torch.isfinite(getattr(b, n)).all(), (ck.tag, n)
            ck.within("bwd", n, getattr(b, n), getattr(ref, n))
    if case.exact_dbeta:
        ck.exact("dbeta == integer column sum", b.dbeta, ref.dbeta)


@pytest.mark.parametrize("run", RUNS, ids=IDS)
def test_bn_multi(dev, run):
    from rgbx_semantic_segmentation_amd import kernels as K
    case, dtype, eps = run
    assert K.query("cmx_bn_workspace", case.M, case.C) // (16 * case.C) == case.nblk
    done = []
    for kind in case.kinds:
        exp = nc.bn_expected(case, kind, dtype, eps)
        ck = Checker(case, dtype, eps, kind, exp, "multi")
        d = on_dev(exp.inp, dtype, dev)
        f = multi_fwd(K, d, case, eps, dtype)
        check_fwd(ck, f, exp, case, kind, eps)
        check_bwd(ck, multi_bwd(K, d, case, f, dtype), exp, case)
        done.append(ck)
    nc.finish(done)


@pytest.mark.parametrize("run", RUNS, ids=IDS)
def test_bn_eval(dev, run):
    from rgbx_semantic_segmentation_amd import kernels as K
    case, dtype, eps = run
    done = []
    for kind in case.kinds:
        exp = nc.bn_expected(case, kind, dtype, eps, False)
        ck = Checker(case, dtype, eps, kind, exp, "eval")
        d = on_dev(exp.inp, dtype, dev)
        f = multi_fwd(K, d, case, eps, dtype, training=False)
        check_fwd(ck, f, exp, case, kind, eps, training=False)
        ck.exact("eval leaves the running mean", f.rmean, d.rm0)
        ck.exact("eval leaves the running variance", f.rvar, d.rv0)
        check_bwd(ck, multi_bwd(K, d, case, f, dtype, training=False), exp, case)
        done.append(ck)
    nc.finish(done)


SMALL_RUNS = nc.bn_runs([c for c in nc.BN_CASES if c.small])


@pytest.mark.parametrize("run", SMALL_RUNS, ids=[run_id(r) for r in SMALL_RUNS])
def test_bn_small(dev, run):
    from rgbx_semantic_segmentation_amd import kernels as K
    case, dtype, eps = run
    done = []
    for kind in case.kinds:
        exp = nc.bn_expected(case, kind, dtype, eps)
        ck = Checker(case, dtype, eps, kind, exp, "small")
        d = on_dev(exp.inp, dtype, dev)
        f = small_fwd(K, d, case, eps, dtype)
        check_fwd(ck, f, exp, case, kind, eps)
        b = small_bwd(K, d, case, f, dtype)
        check_bwd(ck, b, exp, case)
        # against the multi-launch path on the same inputs
        fm = multi_fwd(K, d, case, eps, dtype)
        bm = multi_bwd(K, d, case, fm, dtype)
        ck.close64("small vs multi sum x", f.sums[0], fm.sums[0].cpu(), exp.inp.x.abs().sum(0))
        ck.close64("small vs multi sum x^2", f.sums[1], fm.sums[1].cpu(), (exp.inp.x ** 2).sum(0))
        for n in ("mean", "invstd"):
            a, m = getattr(f, n).cpu().double(), getattr(fm, n).cpu().double()
            off = ((a - m).abs() / m.abs().clamp_min(nc.TINY)).max().item()
            print(f"[norm] bn {ck.tag} | small vs multi {n} off by {off:.3e}")
            if not off <= 2.0 ** -23:
                ck.bad.append(("small vs multi", n, off))
        ck.within("small vs multi", "y", f.y, fm.y.double())
        ck.within("small vs multi", "dx", b.dx, bm.dx.double())
        done.append(ck)
    nc.finish(done)


def ints(C, dev, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-9, 10, (C,), generator=g).float().to(dev)


@pytest.mark.parametrize("run", RUNS, ids=IDS)
def test_bn_accumulate(dev, run):
    from rgbx_semantic_segmentation_amd import kernels as K
    case, dtype, eps = run
    kind, code = case.kinds[0], nc.dtype_code(dtype)
    exp = nc.bn_expected(case, kind, dtype, eps)
    ck = Checker(case, dtype, eps, kind, exp, "accumulate")
    d = on_dev(exp.inp, dtype, dev)
    f = multi_fwd(K, d, case, eps, dtype)
    b0 = multi_bwd(K, d, case, f, dtype)
    pg, pb = ints(case.C, dev, 3), ints(case.C, dev, 4)
    dg, db = pg.clone(), pb.clone()
    sums = bwd_reduce(K, d.dy, d.x, d.res, d.dscale, d, f.mean, f.invstd, case, code, dg, db, accumulate=1)
    ck.exact("bn_bwd_reduce accumulate dgamma", dg, pg + b0.dgamma)
    ck.exact("bn_bwd_reduce accumulate dbeta", db, pb + b0.dbeta)
    ck.exact("bn_bwd_reduce accumulate sums", sums, b0.sums)
    assert not torch.equal(dg, b0.dgamma) and not torch.equal(db, b0.dbeta)
    if case.small:
        fs = small_fwd(K, d, case, eps, dtype)
        s0 = small_bwd(K, d, case, fs, dtype)
        dg, db = pg.clone(), pb.clone()
        s1 = small_bwd(K, d, case, fs, dtype, dg, db, accumulate=1)
        ck.exact("bn_small_bwd accumulate dgamma", dg, pg + s0.dgamma)
        ck.exact("bn_small_bwd accumulate dbeta", db, pb + s0.dbeta)
        ck.exact("bn_small_bwd accumulate dx", s1.dx, s0.dx)
    nc.finish([ck])


SYNC_RUNS = nc.bn_runs(nc.BN_SYNC)


@pytest.mark.parametrize("run", SYNC_RUNS, ids=[run_id(r) for r in SYNC_RUNS])
def test_bn_syncbn_two_shards(dev, run):
    from rgbx_semantic_segmentation_amd import kernels as K
    case, dtype, eps = run
    M, C, code = case.M, case.C, nc.dtype_code(dtype)
    m1 = case.rps * (case.nsamp // 2) if M > case.rps else M // 2          # a sample boundary: dscale splits too
    assert 0 < m1 < M
    done = []
    for kind in case.kinds:
        exp = nc.bn_expected(case, kind, dtype, eps)
        ck = Checker(case, dtype, eps, kind, exp, "sync")
        d = on_dev(exp.inp, dtype, dev)
        shards = []
        for lo, hi in ((0, m1), (m1, M)):
            cut = lambda t: None if t is None else t[lo:hi]  # noqa: E731
            shards.append(SimpleNamespace(x=d.x[lo:hi], dy=d.dy[lo:hi], res=cut(d.res),
                                          dscale=dscale_of(d, lo if M > case.rps else 0, case)))
        total = torch.zeros(2, C, dtype=F64, device=dev)
        for s in shards:
            part = torch.empty(2, C, dtype=F64, device=dev)
            K.call("cmx_bn_stats", K.ptr(s.x), K.ptr(part), K.ptr(bn_ws(K, s.x.shape[0], C, dev)), s.x.shape[0], C, code,
                   K.stream())
            total += part
        mean, invstd, rm, rv = f32(C, dev), f32(C, dev), d.rm0.clone(), d.rv0.clone()
        K.call("cmx_bn_finalize", K.ptr(total), float(M), float(eps), case.momentum, K.ptr(rm), K.ptr(rv), K.ptr(mean),
               K.ptr(invstd), C, 1, K.stream())
        y = torch.cat([apply_fwd(K, s.x, s.res, s.dscale, d, mean, invstd, case, code) for s in shards])
        check_fwd(ck, SimpleNamespace(y=y, mean=mean, invstd=invstd, rmean=rm, rvar=rv, sums=total), exp, case, kind, eps)
        gsum, dgs, dbs = torch.zeros(2, C, dtype=F64, device=dev), [], []
        for s in shards:
            dgs.append(f32(C, dev))
            dbs.append(f32(C, dev))
            gsum += bwd_reduce(K, s.dy, s.x, s.res, s.dscale, d, mean, invstd, case, code, dgs[-1], dbs[-1])
        outs = [bwd_apply(K, s.dy, s.x, s.res, s.dscale, d, mean, invstd, gsum, M, case, code) for s in shards]
        b = SimpleNamespace(dx=torch.cat([o[0] for o in outs]),
                            dres=torch.cat([o[1] for o in outs]) if d.res is not None else None,
                            dgamma=dgs[0].double() + dgs[1].double(), dbeta=dbs[0].double() + dbs[1].double())
        check_bwd(ck, b, exp, case)
        done.append(ck)
    nc.finish(done)


# --------------------------------------------------------------------------------- containment
Guard = nc.Guard
CONTAIN = [(c, dt) for c in nc.BN_CONTAINMENT for dt in c.dtypes]


@pytest.mark.parametrize("run", CONTAIN, ids=[f"{c.name}-{nc.name_of(dt)}" for c, dt in CONTAIN])
def test_bn_containment(dev, run):
    from rgbx_semantic_segmentation_amd import kernels as K
    case, dtype = run
    eps, code, M, C = nc.BN_EPS[0], nc.dtype_code(dtype), case.M, case.C
    exp = nc.bn_expected(case, case.kinds[0], dtype, eps)
    d = on_dev(exp.inp, dtype, dev)
    p, act = K.ptr, ACT[case.act]
    f0 = multi_fwd(K, d, case, eps, dtype)
    b0 = multi_bwd(K, d, case, f0, dtype)
    g = lambda n, dt, init=None: Guard(n, dt, dev, init)  # noqa: E731
    y, dx, dres = g(M * C, dtype), g(M * C, dtype), g(M * C, dtype)
    sums, gsums = g(2 * C, F64), g(2 * C, F64)
    mean, invstd, dg, db = (g(C, torch.float32) for _ in range(4))
    rm, rv = g(C, torch.float32, d.rm0), g(C, torch.float32, d.rv0)
    nbytes = K.query("cmx_bn_workspace", M, C)
    assert nbytes == case.nblk * 2 * C * 8
    ws, ws2 = g(nbytes // 8, F64), g(nbytes // 8, F64)
    K.call("cmx_bn_stats_finalize", p(d.x), sums.ptr(), ws.ptr(), M, C, float(eps), case.momentum, rm.ptr(), rv.ptr(),
           mean.ptr(), invstd.ptr(), code, K.stream())
    K.call("cmx_bn_apply", p(d.x), mean.ptr(), invstd.ptr(), p(d.gamma), p(d.beta), p(d.res), p(d.dscale), y.ptr(), M, C,
           case.rps, act, code, K.stream())
    K.call("cmx_bn_bwd_reduce", p(d.dy), p(d.x), mean.ptr(), invstd.ptr(), p(d.gamma), p(d.beta), p(d.res), p(d.dscale),
           gsums.ptr(), dg.ptr(), db.ptr(), ws2.ptr(), M, C, case.rps, act, 0, code, K.stream())
    K.call("cmx_bn_bwd_apply", p(d.dy), p(d.x), mean.ptr(), invstd.ptr(), p(d.gamma), p(d.beta), p(d.res), p(d.dscale),
           gsums.ptr(), float(M), dx.ptr(), dres.ptr() if d.res is not None else 0, M, C, case.rps, act, 1, code,
           K.stream())
    torch.cuda.synchronize()
    guards = dict(y=y, dx=dx, dres=dres, sums=sums, gsums=gsums, mean=mean, invstd=invstd, dgamma=dg, dbeta=db,
                  rmean=rm, rvar=rv, workspace=ws, workspace_bwd=ws2)
    for name, t in guards.items():
        assert t.intact(), f"{case.name}: a store outside the logical {name}"
    if d.res is None:
        assert (dres.view == nc.SENTINEL).all()
    packed = dict(y=f0.y, dx=b0.dx, dres=b0.dres, sums=f0.sums, gsums=b0.sums, mean=f0.mean, invstd=f0.invstd,
                  dgamma=b0.dgamma, dbeta=b0.dbeta, rmean=f0.rmean, rvar=f0.rvar)
    for name, t in packed.items():
        if t is not None:
            assert torch.equal(guards[name].view.view(t.shape), t), (case.name, name)
    if not case.small:
        return
    fs0 = small_fwd(K, d, case, eps, dtype)
    bs0 = small_bwd(K, d, case, fs0, dtype)
    y, dx, dres = g(M * C, dtype), g(M * C, dtype), g(M * C, dtype)
    sums = g(2 * C, F64)
    mean, invstd, dg, db = (g(C, torch.float32) for _ in range(4))
    rm, rv = g(C, torch.float32, d.rm0), g(C, torch.float32, d.rv0)
    K.call("cmx_bn_small_fwd", p(d.x), p(d.res), p(d.gamma), p(d.beta), p(d.dscale), y.ptr(), sums.ptr(), mean.ptr(),
           invstd.ptr(), rm.ptr(), rv.ptr(), M, C, case.rps, act, float(eps), case.momentum, code, K.stream())
    K.call("cmx_bn_small_bwd", p(d.dy), p(d.x), mean.ptr(), invstd.ptr(), p(d.gamma), p(d.beta), p(d.res), p(d.dscale),
           dg.ptr(), db.ptr(), dx.ptr(), dres.ptr() if d.res is not None else 0, M, C, case.rps, act, 0, code, K.stream())
    torch.cuda.synchronize()
    guards = dict(y=y, dx=dx, dres=dres, sums=sums, mean=mean, invstd=invstd, dgamma=dg, dbeta=db, rmean=rm, rvar=rv)
    for name, t in guards.items():
        assert t.intact(), f"{case.name}: small path, a store outside the logical {name}"
    packed = dict(y=fs0.y, dx=bs0.dx, dres=bs0.dres, sums=fs0.sums, mean=fs0.mean, invstd=fs0.invstd, dgamma=bs0.dgamma,
                  dbeta=bs0.dbeta, rmean=fs0.rmean, rvar=fs0.rvar)
    for name, t in packed.items():
        if t is not None:
            assert torch.equal(guards[name].view.view(t.shape), t), (case.name, "small", name)
