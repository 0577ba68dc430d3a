"""Inputs, references and yardstick of the LayerNorm and BatchNorm tests: one table of cases per
family, read by tests/test_norm_cases.py (CPU: the constructions hold on the references alone, every
LayerNorm case lands on the launch plan it names) and by tests/test_gpu_layernorm.py and
tests/test_gpu_batchnorm.py (GPU: every kernel variant against fp64).

References.  fp64 torch on the inputs as rounded to the storage type.  LayerNorm: y, per-row mean and
rstd, and the autograd backward of LN(x) under upstream dy + dy2, dx += dres, dxs = sscale[sample] dx.
BatchNorm: y = act(BN(x) + res) dscale, mean / invstd / running statistics (momentum, unbiased
variance), and the autograd dx / dres / dgamma / dbeta, train and eval.

Input kinds (for BatchNorm read "row" as "channel").
  random  N(0.5, 2^2).
  offset  64 + k s, integer k in [-8, 8], s = 1/8 (1/2 in bf16): values exact in the storage type and a
          mean 100 x the spread.  A one-pass fp32 variance E[x^2] - mean^2 rounds E[x^2] ~ 4096 to 2.4e-4,
          which is 6e-4 of the variance; the two-pass form does not.
  tiny    1 + k u, k in {-1, 0, 1}, u the storage spacing at 1 (2^-10 fp32 / fp16, 2^-7 bf16): the variance
          is of the order of eps, so 1e-6 in place of 1e-5 moves y by 5e-2 .. 3e-1 of the row scale.  In
          bf16 seven k in eight are 0: at uniform k the variance (4e-5) is above both eps values and the
          swap moves y by 6e-2, only 5 x the bf16 bound of 3 x 2^-8.  For BatchNorm the step follows eps
          (2^-8 at 1e-5, 2^-7 in bf16; 2^-5 at 1e-3), k uniform.
  const   every element of the row one small integer: y = beta rounded to the storage type and mean = the
          constant, exactly, rstd = eps^-1/2 (LayerNorm: x - mean is exactly 0).  BatchNorm also holds one
          constant channel at 0.1 (not dyadic: E[x^2] - mean^2 rounds to either side of 0 in fp64, the
          `var < 0` clamp).
Gradients dy, dy2, dres are integers of [-4, 4]: every column sum of dy + dy2 is an integer below 2^24, so
dbeta is exact in fp32 in any summation order (BatchNorm: with act = none and dscale in {0, 2}).  sscale
holds {0, 0.5, 1, 2} and one sample at 1.25: a power of two commutes with the storage rounding, so there
dxs == sscale dx on the stored tensors exactly.

Yardstick.  emulate_* is the fp32 CPU restatement of the kernel's arithmetic (LayerNorm: two-pass mean and
variance, rsqrt, affine; BatchNorm: x sc + sh from fp64 statistics; both: the backward formulas of the
kernel comments), evaluated with two summation orders, sequential and torch's pairwise sum.  E_emul is its
larger error against fp64: per row (LayerNorm) or per channel (BatchNorm) the maximum error over the
row / channel divided by its max |ref|, then the maximum over rows / channels; per tensor for dgamma,
dbeta, mean, rstd, invstd and the running statistics.  The GPU bound is FACTOR E_emul + u with FACTOR = 2
(two correct fp32 summation orders each lie within E of fp64, so within 2 E of one another) and u one unit
of the output type relative to the same scale: 2^-8 bf16, 2^-11 fp16, 2^-22 for fp32 outputs (the
hardware rsqrt and the final rounding).

BatchNorm's forward has no sum in it, so its two evaluations differ in the other freedom a correct fp32
evaluation of x sc + sh has: separate roundings, or sh and x sc + sh as one fused multiply-add each, which is
what the device compiler's contraction makes of the kernel source.  With separate roundings a constant channel
cancels exactly (fl(x sc) == fl(mean sc)); fused, it keeps the rounding of sh, up to 2^-24 |mean sc|, which at
eps = 1e-3 and |beta| ~ 0.02 is 2.9e-3 of the channel's |y|.  The separate-rounding emulation alone put E_emul
at 6e-5 .. 4e-4 on those channels and the kernels measured 7.9e-4 .. 2.9e-3 (up to 6.4 x that bound); the
fused emulation reproduces the measured figures to every printed digit."""
from __future__ import annotations

import functools
import math
from collections import namedtuple
from dataclasses import dataclass

import torch

FACTOR = 2
BF16, FP16, FP32 = torch.bfloat16, torch.float16, torch.float32
H16, F32 = (BF16, FP16), (FP32,)
ULP = {BF16: 2.0 ** -8, FP16: 2.0 ** -11, FP32: 2.0 ** -22}
ULP32 = 2.0 ** -22                                 # fp32 outputs of every dtype: statistics, dgamma, dbeta
KINDS = ("random", "offset", "tiny", "const")
LN_EPS = (1e-6, 1e-5)                              # block / stage norms; patch-embed, SR and CrossPath norms
BN_EPS = (1e-5, 1e-3)                              # ChannelEmbed BNs; the decoder's linear_fuse BN
SENTINEL = -3072.0                                 # exact in bf16 / fp16 / fp32
TINY = 1e-300
ORDERS = ("seq", "pair")


def vec_width(dtype):
    return 4 if dtype == FP32 else 8


def dtype_code(dtype):
    return {FP32: 0, BF16: 1, FP16: 2}[dtype]


def name_of(dtype):
    return str(dtype).replace("torch.", "")


def bound(e_emul, u):
    return FACTOR * e_emul + u


def rowerr(a, ref, dim=-1):
    """max over rows (dim = -1) or channels (dim = 0) of the row's max error over its max |ref|"""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return ((a - ref).abs().amax(dim) / ref.abs().amax(dim).clamp_min(TINY)).max().item()


def tenerr(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return ((a - ref).abs().max() / ref.abs().max().clamp_min(TINY)).item()


def _sum(t, dim, order):
    if order == "pair":
        return t.sum(dim)
    t = t.movedim(dim, 0)
    acc = torch.zeros_like(t[0])
    for i in range(t.shape[0]):
        acc += t[i]
    return acc


def _seed(*parts):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate("|".join(str(p) for p in parts))) * 7919 % (2 ** 31)


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


# ================================================================================== LayerNorm
@dataclass(frozen=True, eq=False)                  # cases are module-level singletons: identity hash
class LnCase:
    name: str
    R: int
    G: int
    C: int
    dtypes: tuple
    fwd: tuple                                     # (tpr, nch, rpt) of ln_fwd_kernel the case is meant for
    bwd: tuple                                     # ... of ln_bwd_kernel
    rps: int = 37                                  # rows per sample of sscale (no multiple of a block's rows)
    kinds: tuple = KINDS

    @property
    def rows(self):
        return self.G * self.R

    @property
    def nsamp(self):
        return -(-self.rows // self.rps)


LN_FWD_PLANS = ((4, 1, 4), (8, 1, 4), (16, 1, 4), (4, 1, 1), (8, 1, 1), (16, 1, 1), (32, 1, 1), (64, 1, 1), (64, 2, 1),
                (64, 4, 1))
LN_BWD_PLANS = tuple((t, n, 2 if r == 4 else 1) for t, n, r in LN_FWD_PLANS)
BIG = ("random", "offset")                         # the 2 M-element cases: two kinds


def _ln_cases():
    c = []

    def add(name, R, G, C, dtypes, plan, big=False, **kw):
        fwd = plan + (4 if big else 1,)
        c.append(LnCase(name, R, G, C, dtypes, fwd, plan + (2 if big else 1,), **kw))

    # rows per thread > 1: the smallest R that selects it (forward R G >= 1024 rpb, backward R > 512 rpb),
    # + 37 so the last block is ragged in the row slot and in the rpt index
    add("rpt_tpr4_C24_bf16", 65536 + 37, 1, 24, (BF16,), (4, 1), big=True, kinds=BIG + ("tiny",))
    add("rpt_tpr8_C40_fp16_G2", 16384 + 37, 2, 40, (FP16,), (8, 1), big=True, kinds=BIG)
    add("rpt_tpr16_C64_f32", 16384 + 37, 1, 64, F32, (16, 1), big=True, kinds=BIG)
    # 16-bit: ragged chunk counts (C = 8, 24: idle lanes at tpr 4), G = 2 with a sample across the group boundary
    add("h16_C8", 185, 2, 8, H16, (4, 1), rps=74)
    add("h16_C24", 185, 2, 24, H16, (4, 1), rps=74)
    add("h16_C40", 185, 2, 40, H16, (8, 1), rps=74)
    add("h16_C64", 111, 1, 64, H16, (8, 1))
    add("h16_C160", 185, 2, 160, H16, (32, 1), rps=74)
    add("h16_C320", 185, 2, 320, H16, (64, 1), rps=74)
    add("h16_C512", 37, 1, 512, H16, (64, 1))
    add("h16_C640", 37, 1, 640, H16, (64, 2))
    add("h16_C1024_G2", 74, 2, 1024, H16, (64, 2))                       # the backward's two-pass LDS fold
    # one block's rows - 1, + 1 and a single row at a narrow, a medium and a wide C
    for R in (1, 63, 65):
        add(f"h16_C32_R{R}", R, 1, 32, H16, (4, 1))
    for R in (1, 15, 17):
        add(f"h16_C128_R{R}", R, 1, 128, H16, (16, 1))
    for R in (1, 3, 5):
        add(f"h16_C1024_R{R}", R, 1, 1024, H16, (64, 2))
    # the backward's grid-stride loop at rpt = 1: 512 blocks of 8 rows and 37 rows more
    add("h16_C256_stride", 4096 + 37, 1, 256, H16, (32, 1), kinds=("random", "offset", "const"))
    # fp32
    add("f32_C12", 185, 2, 12, F32, (4, 1), rps=74)
    add("f32_C32", 111, 1, 32, F32, (8, 1))
    add("f32_C128", 111, 1, 128, F32, (32, 1))
    add("f32_C160", 185, 2, 160, F32, (64, 1), rps=74)
    add("f32_C320", 185, 2, 320, F32, (64, 2), rps=74)
    add("f32_C640_G2", 74, 2, 640, F32, (64, 4))                         # three chunks per lane: the NCH = 4 kernels
    add("f32_C768", 37, 1, 768, F32, (64, 4))
    add("f32_C1024_G2", 74, 2, 1024, F32, (64, 4))
    for R in (1, 63, 65):
        add(f"f32_C16_R{R}", R, 1, 16, F32, (4, 1))
    for R in (1, 15, 17):
        add(f"f32_C64_R{R}", R, 1, 64, F32, (16, 1))
    for R in (1, 3, 5):
        add(f"f32_C1024_R{R}", R, 1, 1024, F32, (64, 4))
    return c


LN_CASES = _ln_cases()


def _one_per_plan():
    seen, out = set(), []
    for c in LN_CASES:
        if c.R > 1 and (c.fwd, c.bwd) not in seen:
            seen.add((c.fwd, c.bwd))
            out.append(c)
    return out


LN_CONTAINMENT = _one_per_plan()


def ln_runs(cases=None):
    return [(c, dt, eps) for c in (LN_CASES if cases is None else cases) for dt in c.dtypes for eps in LN_EPS]


def ln_run_id(r):
    c, dt, eps = r
    return f"{c.name}-{name_of(dt)}-eps{eps:g}"


LnInputs = namedtuple("LnInputs", "x gamma beta dy dy2 dres sscale")     # fp64, exact in the storage type / fp32


def kind_values(kind, dtype, g, shape, row_dim, step=None):
    """fp64 values exact in `dtype`; the const kind is constant along every dim but `row_dim`"""
    if kind == "random":
        return (torch.randn(*shape, generator=g, dtype=torch.float64) * 2 + 0.5).to(dtype).double()
    if kind == "offset":
        return 64.0 + _ints(g, -8, 8, *shape) * (0.5 if dtype == BF16 else 0.125)
    if kind == "tiny":
        k = _ints(g, -1, 1, *shape)
        if step is not None:
            return 1.0 + k * step
        if dtype != BF16:
            return 1.0 + k * 2.0 ** -10
        # bf16's spacing 2^-7 alone gives a variance of 4e-5, above both eps values: one k in eight is
        # non-zero, which brings it to 5e-6
        return 1.0 + k * (_ints(g, 0, 7, *shape) == 0) * 2.0 ** -7
    assert kind == "const", kind
    one = [n if i == row_dim else 1 for i, n in enumerate(shape)]
    return _ints(g, -8, 8, *one).expand(*shape).contiguous()


def sample_scales(n):
    s = torch.tensor([2.0, 0.5, 0.0, 1.0], dtype=torch.float64).repeat(n // 4 + 1)[:n].clone()
    s[min(1, n - 1)] = 1.25
    return s


def pow2_exact(s, dx, dtype):
    """where dxs == s dx must hold bit for bit on the stored tensors: the sample's scale is 0, 1, or a power
    of two with dx and s dx both in the storage type's normal range (a subnormal has no spare bit to halve)"""
    low = torch.finfo(dtype).tiny
    normal = (dx.abs() >= low) & ((s * dx).abs() >= low) & ((s * dx).abs() <= torch.finfo(dtype).max)
    return ((s == 0) | (s == 1) | ((s != 1.25) & (normal | (dx == 0)))).expand_as(dx)


def make_ln_inputs(case, kind, dtype):
    g = torch.Generator().manual_seed(_seed(case.name, kind))
    rows, C, G = case.rows, case.C, case.G
    x = kind_values(kind, dtype, g, (rows, C), 0)
    assert torch.equal(x.to(dtype).double(), x)
    gamma = (1.0 + 0.5 * torch.randn(G, C, generator=g, dtype=torch.float64)).float().double()
    beta = torch.randn(G, C, generator=g, dtype=torch.float64).float().double()
    dy, dy2, dres = (_ints(g, -4, 4, rows, C) for _ in range(3))
    return LnInputs(x, gamma, beta, dy, dy2, dres, sample_scales(case.nsamp))


LnRef = namedtuple("LnRef", "y mean rstd dx1 dg1 db1 dx2 dg2 db2")


def ln_reference(inp, G, eps):
    """fp64: y (rows, C), mean / rstd (rows), and the autograd gradients under dy (1) and under dy2 (2)"""
    rows, C = inp.x.shape
    x = inp.x.clone().requires_grad_(True)
    gam, bet = inp.gamma.clone().requires_grad_(True), inp.beta.clone().requires_grad_(True)
    xg = x.view(G, rows // G, C)
    mean = xg.mean(-1, keepdim=True)
    var = ((xg - mean) ** 2).mean(-1, keepdim=True)
    rstd = (var + eps).rsqrt()
    y = ((xg - mean) * rstd * gam[:, None, :] + bet[:, None, :]).view(rows, C)
    g1 = torch.autograd.grad(y, (x, gam, bet), inp.dy, retain_graph=True)
    g2 = torch.autograd.grad(y, (x, gam, bet), inp.dy2)
    return LnRef(y.detach(), mean.detach().reshape(rows), rstd.detach().reshape(rows), *g1, *g2)


LN_VARIANTS = ("plain", "dy2", "dres", "sscale", "all")
LnBwd = namedtuple("LnBwd", "dx dxs dgamma dbeta")


def _uses(variant):
    return (variant in ("dy2", "all"), variant in ("dres", "all"), variant in ("sscale", "all"))


def sample_of_row(case):
    return torch.arange(case.rows) // case.rps


def ln_expected_bwd(case, inp, ref, variant):
    """the fp64 backward of one cmx_layernorm_bwd_res argument set (the backward is linear in its upstream)"""
    two, res, sc = _uses(variant)
    dx = ref.dx1 + (ref.dx2 if two else 0) + (inp.dres if res else 0)
    dxs = inp.sscale[sample_of_row(case)][:, None] * dx if sc else None
    return LnBwd(dx, dxs, ref.dg1 + (ref.dg2 if two else 0), ref.db1 + (ref.db2 if two else 0))


def emulate_ln_fwd(inp, G, eps, dtype, order, one_pass=False):
    """fp32: mean = sum / C, variance from the centred values, rsqrt, affine; y rounded to `dtype`"""
    rows, C = inp.x.shape
    x = inp.x.float().view(G, rows // G, C)
    mu = _sum(x, -1, order) / C
    if one_pass:
        q = (_sum(x * x, -1, order) / C - mu * mu).clamp_min(0.0)
    else:
        d = x - mu[..., None]
        q = _sum(d * d, -1, order) / C
    rstd = torch.rsqrt(q + eps)
    y = (x - mu[..., None]) * rstd[..., None] * inp.gamma.float()[:, None, :] + inp.beta.float()[:, None, :]
    return y.view(rows, C).to(dtype).double(), mu.reshape(rows), rstd.reshape(rows)


def emulate_ln_bwd(case, inp, dtype, order, mu, rstd, variant, colsums=None):
    """fp32: dx = rstd (g - mean(g) - xhat mean(g xhat)), g = (dy + dy2) gamma, + dres; dxs from the
    unrounded dx; column sums of dv xhat and dv"""
    two, res, sc = _uses(variant)
    G, R, C = case.G, case.R, case.C
    x = inp.x.float().view(G, R, C)
    dv = (inp.dy.float() + (inp.dy2.float() if two else 0)).view(G, R, C)
    xh = (x - mu.view(G, R, 1)) * rstd.view(G, R, 1)
    g = dv * inp.gamma.float()[:, None, :]
    s1 = _sum(g, -1, order) / C
    s2 = _sum(g * xh, -1, order) / C
    o = rstd.view(G, R, 1) * (g - s1[..., None] - xh * s2[..., None])
    if res:
        o = o + inp.dres.float().view(G, R, C)
    dxs = None
    if sc:
        dxs = (o * inp.sscale.float()[sample_of_row(case)].view(G, R, 1)).view(-1, C).to(dtype).double()
    if colsums is None or two not in colsums:          # they depend on the upstream gradient alone
        cs = _sum(torch.cat([dv * xh, dv], -1), 1, order).double().split(C, -1)
        if colsums is not None:
            colsums[two] = cs
    else:
        cs = colsums[two]
    return LnBwd(o.view(-1, C).to(dtype).double(), dxs, *cs)


LnExpected = namedtuple("LnExpected", "inp ref e")    # e: {tensor or (variant, tensor): E_emul}


@functools.lru_cache(maxsize=None)
def ln_expected(case, kind, dtype, eps):
    """inputs, fp64 reference and E_emul of one run: computed once, shared by the tests, never modified"""
    inp = make_ln_inputs(case, kind, dtype)
    ref = ln_reference(inp, case.G, eps)
    e = {}

    def worse(key, val):
        e[key] = max(e.get(key, 0.0), val)

    for order in ORDERS:
        y, mu, rs = emulate_ln_fwd(inp, case.G, eps, dtype, order)
        worse("y", rowerr(y, ref.y))
        worse("mean", tenerr(mu, ref.mean))
        worse("rstd", tenerr(rs, ref.rstd))
        colsums = {}
        for variant in LN_VARIANTS:
            want = ln_expected_bwd(case, inp, ref, variant)
            got = emulate_ln_bwd(case, inp, dtype, order, mu, rs, variant, colsums)
            worse((variant, "dx"), rowerr(got.dx, want.dx))
            if want.dxs is not None:
                worse((variant, "dxs"), rowerr(got.dxs, want.dxs))
            worse((variant, "dgamma"), tenerr(got.dgamma, want.dgamma))
            worse((variant, "dbeta"), tenerr(got.dbeta, want.dbeta))
    return LnExpected(inp, ref, e)


def ln_bound(exp, key, dtype):
    name = key[1] if isinstance(key, tuple) else key
    return bound(exp.e[key], ULP[dtype] if name in ("y", "dx", "dxs") else ULP32)


# ================================================================================== BatchNorm
@dataclass(frozen=True, eq=False)
class BnCase:
    name: str
    M: int
    C: int
    dtypes: tuple
    act: str = "none"
    res: bool = False
    dscale: bool = False
    small: bool = False                            # also eligible for cmx_bn_small_* (C % 16 == 0, M <= 600)
    rps: int = 37                                  # rows per sample of dscale
    kinds: tuple = KINDS
    momentum: float = 0.1

    @property
    def nblk(self):
        return min(256, max(1, -(-self.M // 16)))

    @property
    def tpr(self):
        t, chunks = 4, self.C // vec_width(self.dtypes[0])
        while t < chunks and t < 32:
            t <<= 1
        return t

    @property
    def nsamp(self):
        return -(-self.M // self.rps)

    @property
    def exact_dbeta(self):
        return self.act == "none"


def _bn_cases():
    c = []
    opts = [dict(act=a, res=r, dscale=d) for a in ("none", "relu") for r in (False, True) for d in (False, True)]
    # every option set on one shape per vector width (lane width 8 / 16)
    for i, o in enumerate(opts):
        tag = f"{o['act']}{'_res' if o['res'] else ''}{'_ds' if o['dscale'] else ''}"
        c.append(BnCase(f"opt_{tag}_h16", 277, 64, H16, **o))
        c.append(BnCase(f"opt_{tag}_f32", 277, 64, F32, **o))
    # lane widths 4 .. 32 with the ragged channel counts; options in rotation
    for i, (C, dts) in enumerate([(16, F32), (32, F32), (136, F32), (8, H16), (32, H16), (128, H16), (136, H16),
                                  (512, H16)]):
        c.append(BnCase(f"lanes_C{C}_{'f32' if dts == F32 else 'h16'}", 277, C, dts, **opts[(3 * i + 1) % 8]))
    # row-block counts that end the fold's three loops at different places: 1, 2, 18 (above), 65, 250, the cap
    for M in (2, 17, 1031, 3989, 5003):
        kinds = KINDS if M < 3000 else ("random", "offset", "const")
        c.append(BnCase(f"rows_M{M}_C32_f32", M, 32, F32, res=M % 2 == 1, dscale=M > 1000, kinds=kinds))
        c.append(BnCase(f"rows_M{M}_C136_h16", M, 136, H16, res=M % 2 == 0, dscale=M < 1000, kinds=kinds))
    # the one-launch small path (and the multi-launch path on the same inputs)
    for i, (M, C) in enumerate([(2, 16), (63, 16), (600, 16), (2, 512), (63, 512), (600, 512)]):
        o = opts[(3 * i) % 8]
        c.append(BnCase(f"small_M{M}_C{C}_h16", M, C, H16, small=True, **o))
        c.append(BnCase(f"small_M{M}_C{C}_f32", M, C, F32, small=True, **opts[(3 * i + 2) % 8]))
    return c


BN_CASES = _bn_cases()
BN_CONTAINMENT = [c for c in BN_CASES if c.name in ("lanes_C136_f32", "lanes_C136_h16", "lanes_C8_h16",
                                                    "opt_relu_res_ds_h16", "rows_M5003_C32_f32",
                                                    "small_M63_C16_h16", "small_M600_C512_f32")]
BN_SYNC = [c for c in BN_CASES if c.name.startswith(("opt_none", "opt_relu_res_ds", "rows_M1031", "rows_M17"))]


def bn_runs(cases=None):
    return [(c, dt, eps) for c in (BN_CASES if cases is None else cases) for dt in c.dtypes for eps in BN_EPS]


def bn_tiny_step(dtype, eps):
    if eps >= 1e-3:
        return 2.0 ** -5
    return 2.0 ** -7 if dtype == BF16 else 2.0 ** -8


RELU_MARGIN = 2e-3       # no pre-activation of a relu case lies closer to 0 (train or eval): see make_bn_inputs
BnInputs = namedtuple("BnInputs", "x gamma beta res dscale dy rm0 rv0")


def _bn_pre(x, gamma, beta, res, mean, invstd):
    pre = (x - mean) * invstd * gamma + beta
    return pre + res if res is not None else pre


@functools.lru_cache(maxsize=None)
def make_bn_inputs(case, kind, dtype, eps):
    """fp64 values exact in `dtype` (x, res, dy) or fp32.  relu cases: beta is moved, per channel, in steps
    of 1/64 until no pre-activation (of the training and of the eval forward) lies within RELU_MARGIN of
    0, where fp32 and fp64 may disagree on the derivative's branch (the const kind's x sc is ~2500, one
    fp32 ulp of which is 2.4e-4)"""
    g = torch.Generator().manual_seed(_seed(case.name, kind))
    M, C = case.M, case.C
    x = kind_values(kind, dtype, g, (M, C), 1, step=bn_tiny_step(dtype, eps))
    if kind == "const" and C > 1:
        x[:, 1] = torch.tensor(0.1, dtype=torch.float64).to(dtype).double()
    assert torch.equal(x.to(dtype).double(), x)
    gamma = (1.0 + 0.5 * torch.randn(C, generator=g, dtype=torch.float64)).float().double()
    beta = torch.randn(C, generator=g, dtype=torch.float64).float().double()
    res = torch.randn(M, C, generator=g, dtype=torch.float64).to(dtype).double() if case.res else None
    dscale = 2.0 * _ints(g, 0, 1, case.nsamp, C) if case.dscale else None
    dy = _ints(g, -4, 4, M, C)
    rm0 = (0.5 * torch.randn(C, generator=g, dtype=torch.float64) + (0.0 if kind == "random" else x.mean())) \
        .float().double()
    rv0 = (0.5 + torch.rand(C, generator=g, dtype=torch.float64)).float().double()
    if case.act == "relu":
        mean, var = x.mean(0), x.var(0, unbiased=False)
        pres = [_bn_pre(x, gamma, 0.0, res, mean, (var + eps).rsqrt()), _bn_pre(x, gamma, 0.0, res, rm0, (rv0 + eps).rsqrt())]
        shift = torch.arange(256, dtype=torch.float64) / 64
        ok = torch.ones(256, C, dtype=torch.bool)
        for p in pres:
            for j in range(256):
                ok[j] &= ((p + (beta + shift[j])).abs() > RELU_MARGIN).all(0)
        assert ok.any(0).all(), case.name
        beta = (beta + shift[ok.int().argmax(0)]).float().double()
        for p in pres:
            assert ((p + beta).abs() > RELU_MARGIN / 2).all(), case.name
    return BnInputs(x, gamma, beta, res, dscale, dy, rm0, rv0)


BnRef = namedtuple("BnRef", "y mean invstd rmean rvar dx dres dgamma dbeta")


def _act(pre, act):
    return pre.clamp_min(0.0) if act == "relu" else pre


def _rows(dscale, M, rps):
    return dscale[torch.arange(M) // rps]


def bn_reference(case, inp, eps, training=True, shards=None):
    """fp64 autograd.  Eval: mean / invstd from rm0 / rv0, which stay as they are."""
    M, C = inp.x.shape
    x = inp.x.clone().requires_grad_(True)
    gam, bet = inp.gamma.clone().requires_grad_(True), inp.beta.clone().requires_grad_(True)
    res = inp.res.clone().requires_grad_(True) if inp.res is not None else None
    if training:
        mean = x.mean(0)
        var = ((x - mean) ** 2).mean(0)
        rmean = (1 - case.momentum) * inp.rm0 + case.momentum * mean.detach()
        rvar = (1 - case.momentum) * inp.rv0 + case.momentum * var.detach() * (M / (M - 1) if M > 1 else 1.0)
    else:
        mean, var, rmean, rvar = inp.rm0, inp.rv0, inp.rm0, inp.rv0
    invstd = (var + eps).rsqrt()
    y = _act(_bn_pre(x, gam, bet, res, mean, invstd), case.act)
    if inp.dscale is not None:
        y = y * _rows(inp.dscale, M, case.rps)
    gr = torch.autograd.grad(y, (x, gam, bet) + ((res,) if res is not None else ()), inp.dy)
    return BnRef(y.detach(), mean.detach(), invstd.detach(), rmean, rvar, gr[0], gr[3] if res is not None else None,
                 gr[1], gr[2])


def _fma(a, b, c):
    """fp32 fused multiply-add (the product of two fp32 values is exact in fp64)"""
    return (a.double() * b.double() + c.double()).float()


def emulate_bn(case, inp, eps, dtype, order, training=True, fused=False):
    """fp32 from fp64 statistics: y = act(x sc + sh + res) dscale with sc = gamma invstd, sh = beta - mean sc;
    g = dy dscale act'(pre), sums of g and g xhat, dx = sc (g - sum_g / M - xhat sum_gx / M) (eval: sc g).
    fused: sh and x sc + sh as one fused multiply-add each, the other correct fp32 evaluation of the same
    expressions (what the device compiler's contraction makes of them)"""
    M, C = inp.x.shape
    x = inp.x.float()
    if training:
        mean64 = inp.x.mean(0)
        var64 = ((inp.x - mean64) ** 2).mean(0)
        mean, invstd = mean64.float(), (var64 + float(torch.tensor(eps).float())).rsqrt().float()
        unb = var64 * (M / (M - 1) if M > 1 else 1.0)
        rmean = ((1 - case.momentum) * inp.rm0 + case.momentum * mean64).float()
        rvar = ((1 - case.momentum) * inp.rv0 + case.momentum * unb).float()
    else:
        mean, invstd = inp.rm0.float(), 1.0 / torch.sqrt(inp.rv0.float() + eps)
        rmean, rvar = inp.rm0.float(), inp.rv0.float()
    sc = inp.gamma.float() * invstd
    sh = _fma(-mean, sc, inp.beta.float()) if fused else inp.beta.float() - mean * sc
    pre = _fma(x, sc, sh.expand_as(x)) if fused else x * sc + sh
    if inp.res is not None:
        pre = pre + inp.res.float()
    ds = _rows(inp.dscale, M, case.rps).float() if inp.dscale is not None else None
    y = _act(pre, case.act)
    g = inp.dy.float() * ((pre > 0).float() if case.act == "relu" else 1.0)
    if ds is not None:
        y, g = y * ds, g * ds
    xh = (x - mean) * invstd
    sg, sgx = _sum(g, 0, order), _sum(g * xh, 0, order)
    dx = sc * (g - sg / M - xh * (sgx / M)) if training else sc * g
    return BnRef(y.to(dtype).double(), mean, invstd, rmean, rvar, dx.to(dtype).double(),
                 g.to(dtype).double() if inp.res is not None else None, sgx.double(), sg.double())


BN_ROWWISE = ("y", "dx", "dres")
BN_FUSED = (False, True)       # the sequential order with separate roundings, the pairwise one with fused x sc + sh
BnExpected = namedtuple("BnExpected", "inp ref e")


@functools.lru_cache(maxsize=None)
def bn_expected(case, kind, dtype, eps, training=True):
    inp = make_bn_inputs(case, kind, dtype, eps)
    ref = bn_reference(case, inp, eps, training)
    e = {}
    for order, fused in zip(ORDERS, BN_FUSED):
        emu = emulate_bn(case, inp, eps, dtype, order, training, fused)
        for n in BnRef._fields:
            a, b = getattr(emu, n), getattr(ref, n)
            if b is not None:
                e[n] = max(e.get(n, 0.0), rowerr(a, b, 0) if n in BN_ROWWISE else tenerr(a, b))
    return BnExpected(inp, ref, e)


def bn_bound(exp, n, dtype):
    return bound(exp.e[n], ULP[dtype] if n in BN_ROWWISE else ULP32)


def f32_invstd_of_zero_variance(eps):
    """(float)(1 / sqrt(0 + (double)(float) eps)): what the finalize stores for a constant channel"""
    e = float(torch.tensor(eps, dtype=torch.float32))
    return float(torch.tensor(1.0 / math.sqrt(e), dtype=torch.float64).float())


# ==================================================================== shared by the two GPU test files
class Checker:
    """the checks of one run ("ln" / "bn"): prints every figure, remembers those that missed"""

    def __init__(self, fam, tag, exp, dtype):
        self.fam, self.tag, self.exp, self.dtype, self.bad = fam, tag, exp, dtype, []

    def _say(self, text):
        print(f"[norm] {self.fam} {self.tag} | {text}")

    def within(self, what, key, got, want):
        name = key[1] if isinstance(key, tuple) else key
        if self.fam == "ln":
            err = rowerr(got, want) if name in ("y", "dx", "dxs") else tenerr(got, want)
            bnd = ln_bound(self.exp, key, self.dtype)
        else:
            err = rowerr(got, want, 0) if name in BN_ROWWISE else tenerr(got, want)
            bnd = bn_bound(self.exp, name, self.dtype)
        self._say(f"{what} {name} err {err:.3e} e_emul {self.exp.e[key]:.3e} bound {bnd:.3e} ratio {err / bnd:.3f}")
        if not err <= bnd:
            self.bad.append((what, name, err, bnd))

    def exact(self, what, got, want):
        same = torch.equal(got.detach().cpu().double(), want.detach().cpu().double())
        self._say(f"{what} exact {same}")
        if not same:
            self.bad.append((what, "not exact"))

    def close64(self, what, got, want, mag):
        err = ((got.detach().cpu() - want).abs() / mag.clamp_min(TINY)).max().item()
        self._say(f"{what} fp64 err {err:.3e}")
        if not err <= 1e-12:
            self.bad.append((what, err))


def finish(checkers):
    """every kind has run and printed: fail with all that missed"""
    bad = [(c.tag, c.bad) for c in checkers if c.bad]
    assert not bad, bad


PAD = 4096                                         # guard elements on either side (a multiple of 16 B)


class Guard:
    """n elements inside a buffer with PAD sentinels before and after (the logical part starts on 16 B)"""

    def __init__(self, n, dtype, dev, init=None):
        self.n = n
        self.buf = torch.full((n + 2 * PAD,), SENTINEL, dtype=dtype, device=dev)
        self.view = self.buf[PAD:PAD + n]
        if init is not None:
            self.view.copy_(init.reshape(-1))
        assert self.view.data_ptr() % 16 == 0

    def ptr(self):
        return self.view.data_ptr()

    def intact(self):
        b = self.buf.cpu()
        return bool((b[:PAD] == SENTINEL).all() and (b[PAD + self.n:] == SENTINEL).all())
