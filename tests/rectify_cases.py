"""Cases, references and yardstick of the cross-modal kernel tests: csrc/frm.hip (combine forward / backward,
pooling backward, the channel-MLP GEMV pair), csrc/ffm_attn.hip (the context softmax) and csrc/ifrm.hip
(mul2, the row LayerNorm, the IFRM combine).  Read by tests/test_rectify_cases.py (CPU: the tables reach every
kernel variant, every exact construction is exact on the references alone) and by tests/test_gpu_frm_kernels.py,
tests/test_gpu_ffm_ctx.py and tests/test_gpu_ifrm_kernels.py (GPU, through the C-ABI).

At kernel level h, sw and cw are given, not computed: no GEMM in front, no ReLU kink moved by it.

References.  Every formula below is one function evaluated in the dtype of its arguments: fp64 is the reference,
fp32 the emulation.  Inputs are rounded to their storage type first.

Yardstick.  E_emul is the largest error against fp64 of the fp32 evaluation over its freedoms: two summation
orders (sequential and torch's pairwise) and, wherever a sigmoid or softmax occurs, two forms of the exponential:
torch.exp, and exp2(fl(x log2 e)) with the product rounded to fp32, which is what __expf lowers to.  The GPU bound
is 2 E_emul + u (norm_cases.py derives the factor 2; the combine backward has a third order, below), u one unit of
the output's storage type relative to the same scale: 2^-8 bf16, 2^-11 fp16, 2^-22 for fp32 outputs.  Errors are
relative to the row's max |ref| for token-major tensors (out, dx, dh, sw, y of rowln; rowln's dx: rowln_err), to the
tensor's max |ref| for the rest.

The combine backward's third order.  With the two orders alone one check of 1 043 missed: db2 of
float16_C32_B3_N67, 5.852e-7 of max |db2| against a bound of 4.648e-7 (E_emul 1.13e-7: sequential 5.9e-8, pairwise
1.13e-7 on the two numbers of db2).  The kernel's reductions are neither order: a lane adds the V values of the
chunks it owns and the lanes fold by halves; a block's row slots stride over the rows, are added in order, and
the per-block fp32 partials are added in fp64 by the test.  That order restated on the CPU in fp32 ("lanes",
_lane_rowsum and _block_partials) gives 5.852172342672456e-07 on that case, the measured figure to every digit: the
kernel evaluates the formula correctly in an order the yardstick did not hold, so frm_expected evaluates the
backward in that order too.  The factor stays 2.

Exact kinds.  Small integers and dyadic factors: every product and every sum is exact in fp32 in any order, so the
value the kernel holds before its store is the fp64 reference itself and the stored tensor is that reference
rounded once to the output type (`ref.to(T)`).  Where the reference is representable in T (the combine outputs
out and dx, the pooling backward, every fp32 output) the rounding is the identity, and the CPU test asserts so;
dh, dsw and da carry up to 24 significant bits and are compared as `ref.to(T)`."""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import torch

FACTOR = 2
BF16, FP16, FP32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = (FP32, BF16, FP16)
ULP = {BF16: 2.0 ** -8, FP16: 2.0 ** -11, FP32: 2.0 ** -22}
ULP32 = 2.0 ** -22
TINY = 1e-300
ORDERS = ("seq", "pair")
FORMS = ("exp", "exp2")
LOG2E = float(torch.tensor(math.log2(math.e), dtype=torch.float32))
ZMAX = 8.0                                         # Gaussian pre-activations of a sigmoid stay within it


def vec_width(dtype):
    return 4 if dtype == FP32 else 8


def name_of(dtype):
    return str(dtype).replace("torch.", "")


def bound(e_emul, u):
    return FACTOR * e_emul + u


def rowerr(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return ((a - ref).abs().amax(-1) / ref.abs().amax(-1).clamp_min(TINY)).max().item()


def tenerr(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return ((a - ref).abs().max() / ref.abs().max().clamp_min(TINY)).item()


def _seed(*parts):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate("|".join(str(p) for p in parts))) * 7919 % (2 ** 31)


def gen(*parts):
    return torch.Generator().manual_seed(_seed(*parts))


def ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def pick(g, values, *shape):
    v = torch.tensor(values, dtype=torch.float64)
    return v[torch.randint(0, len(values), shape, generator=g)]


def randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


def _run(t):
    acc = torch.zeros_like(t[0])
    for i in range(t.shape[0]):
        acc = acc + t[i]
    return acc


def _sum(t, dim, order):
    """pair: torch's sum.  seq: one running sum in index order; above 256 terms, 256 interleaved running sums
    (term i goes to sum i % 256) added in order afterwards, which is also how the kernels' row slots stride"""
    if order == "pair":
        return t.sum(dim)
    t = t.movedim(dim, 0)
    if t.shape[0] > 256:
        pad = (-t.shape[0]) % 256
        if pad:
            t = torch.cat([t, t.new_zeros((pad,) + tuple(t.shape[1:]))])
        t = _run(t.reshape(-1, 256, *t.shape[1:]))
    return _run(t)


def _exp(x, form):
    if x.dtype == torch.float64 or form == "exp":
        return torch.exp(x)
    return torch.exp2(x * LOG2E)                   # the fp32 product is rounded before the exp2


def sigmoid(z, form):
    return 1.0 / (1.0 + _exp(-z, form))


def work(t, dtype):
    """fp64 inputs in the working precision of one evaluation"""
    return None if t is None else t.to(dtype)


# =========================================================== the host-side variant selection, restated
def row_lanes(C, V):
    tpr = 4
    while tpr < C // V and tpr < 64:
        tpr <<= 1
    return tpr


def mch(C, V):
    return 1 if C // V <= row_lanes(C, V) else 2


def rpb_of(C, V):
    return 256 // row_lanes(C, V)


def combine_nblk(N, C, V):
    return min(256, -(-N // rpb_of(C, V)))


def rows_grid(rows, rpb):
    return min(4096, max(1, -(-rows // rpb)))


def pool_bwd_nblk(B, N, C, V):
    return min(-(-N // rpb_of(C, V)), -(-512 // (2 * B)))


IFRM_PPB = 16


def ifrm_nblk(B, N):
    return B * (-(-N // IFRM_PPB))


# =========================================================== FRM combine
@dataclass(frozen=True, eq=False)
class FrmCase:
    name: str
    dtype: torch.dtype
    C: int
    B: int
    N: int
    aim: str                                       # the variant / edge the case is meant for
    kinds: tuple = ("gauss", "exact")
    bwd: bool = True                               # False: a forward-only case (its row count is the forward's matter)

    @property
    def V(self):
        return vec_width(self.dtype)

    @property
    def tpr(self):
        return row_lanes(self.C, self.V)

    @property
    def rpb(self):
        return 256 // self.tpr

    @property
    def mch(self):
        return mch(self.C, self.V)

    @property
    def nblk(self):
        return combine_nblk(self.N, self.C, self.V)

    @property
    def fwd_wraps(self):
        return self.B * self.N > 4096 * self.rpb

    @property
    def bwd_wraps(self):
        return self.N > 256 * self.rpb

    @property
    def partial_second_chunk(self):
        n = self.C // self.V
        return self.tpr == 64 and 64 < n < 128


FRM_C = {BF16: (8, 32, 64, 128, 160, 256, 320, 512, 768, 1024), FP16: (8, 32, 64, 128, 160, 256, 320, 512, 768, 1024),
         FP32: (4, 32, 64, 128, 160, 256, 320, 512)}
FRM_AIM = {(8, 8): "one chunk, three idle lanes", (8, 160): "20 chunks on 32 lanes", (8, 320): "40 chunks on 64 lanes",
           (8, 768): "second chunk half filled, MCH=2", (8, 1024): "second chunk full, MCH=2",
           (4, 4): "one chunk, three idle lanes", (4, 160): "40 chunks on 64 lanes",
           (4, 320): "second chunk partial, MCH=2", (4, 512): "second chunk full, MCH=2"}


def _frm_cases():
    out, turn = [], {}                            # turn: the rotation runs per lane width, over the dtypes
    for dt in DTYPES:
        V = vec_width(dt)
        for i, C in enumerate(FRM_C[dt]):
            rpb = rpb_of(C, V)
            aim = FRM_AIM.get((V, C), f"TPR={row_lanes(C, V)}")
            # each (T, C) at two (B, N): rows straddling images in one block (B = 3, N = 67), and in rotation
            # a single row, one block's rows + 1 and - 1, at B = 1 and B = 8
            out.append(FrmCase(f"{name_of(dt)}_C{C}_B3_N67", dt, C, 3, 67, aim + "; a block's rows straddle images"))
            turn[rpb] = turn.get(rpb, -1) + 1
            B, N = ((8, 1), (1, rpb + 1), (8, rpb - 1), (1, rpb - 1), (8, rpb + 1))[turn[rpb] % 5]
            out.append(FrmCase(f"{name_of(dt)}_C{C}_B{B}_N{N}", dt, C, B, N, aim))
    ex = ("exact",)
    out.append(FrmCase("wrap_bwd_bf16_C512_N1031", BF16, 512, 2, 1031, "backward wraps the grid (N > 256 RPB), TPR=64"))
    out.append(FrmCase("wrap_bwd_bf16_C32_N16391", BF16, 32, 1, 16391, "backward wraps the grid (N > 256 RPB), TPR=4",
                       kinds=ex))
    out.append(FrmCase("wrap_fwd_bf16_C512_BN16389", BF16, 512, 3, 5463, "forward wraps the grid (B N > 4096 RPB), TPR=64",
                       kinds=ex, bwd=False))
    out.append(FrmCase("wrap_fwd_bf16_C32_BN262149", BF16, 32, 1, 262149, "forward wraps the grid (B N > 4096 RPB), TPR=4",
                       kinds=ex, bwd=False))
    out.append(FrmCase("wrap_fwd_fp32_C256_BN16387", FP32, 256, 7, 2341, "forward wraps the grid (B N > 4096 RPB), fp32",
                       kinds=ex, bwd=False))
    out.append(FrmCase("wrap_bwd_fp32_C320_N1029", FP32, 320, 1, 1029, "backward wraps the grid, MCH=2 partial chunk"))
    return out


FRM_CASES = _frm_cases()
FRM_RUNS = [(c, k) for c in FRM_CASES for k in c.kinds]
FRM_BWD_RUNS = [r for r in FRM_RUNS if r[0].bwd]
# exact forward with h > 0 and w2 = 0 (sw = sigmoid(0) = 0.5 through the live branch of the ReLU)
FRM_POS = [c for c in FRM_CASES if c.name in ("bfloat16_C768_B3_N67", "float32_C320_B3_N67", "float16_C8_B3_N67")]


def frm_run_id(r):
    return f"{r[0].name}-{r[1]}"


def frm_fwd(x, cw, h, w2, b2, order="pair", form="exp"):
    """x (2, B, N, C), cw (B, 2C), h (B, N, C), w2 (2, C), b2 (2) -> sw (B, N, 2), out (2, B, N, C)"""
    C = x.shape[-1]
    r = torch.where(h > 0, h, torch.zeros_like(h))
    s = torch.stack([_sum(r * w2[0], -1, order), _sum(r * w2[1], -1, order)], -1) + b2
    sw = sigmoid(s, form)
    c0, c1 = 0.5 * cw[:, None, :C], 0.5 * cw[:, None, C:]
    h0, h1 = 0.5 * sw[..., 0:1], 0.5 * sw[..., 1:2]
    return sw, torch.stack([(x[0] + c1 * x[1]) + h1 * x[1], (x[1] + c0 * x[0]) + h0 * x[0]])


def _lane_rowsum(q, V):
    """sum over C as combine_bwd_kernel forms it: lane l of TPR adds the V values of its chunks l, l + TPR in
    order, then the lanes fold by halves (the xor shuffles of group_sum, seen from lane 0)"""
    C = q.shape[-1]
    tpr, nch = row_lanes(C, V), C // V
    m = -(-nch // tpr)
    qc = q.reshape(*q.shape[:-1], nch, V)
    if m * tpr > nch:
        qc = torch.cat([qc, qc.new_zeros(*q.shape[:-1], m * tpr - nch, V)], -2)
    qc = qc.reshape(*q.shape[:-1], m, tpr, V)
    lane = torch.zeros_like(qc[..., 0, :, 0])
    for k in range(m):
        for j in range(V):
            lane = lane + qc[..., k, :, j]
    w = tpr
    while w > 1:
        w //= 2
        lane = lane[..., :w] + lane[..., w:2 * w]
    return lane[..., 0]


def _block_partials(t, C, V):
    """t (B, N, ...) -> (B, nblk, ...): row n of an image goes to slot n % RPB of block (n / RPB) % nblk, a slot
    adds its rows in order, the slots are added in order (the LDS combine); fp32 throughout"""
    B, N = t.shape[:2]
    rpb, nblk = rpb_of(C, V), combine_nblk(N, C, V)
    pad = (-N) % (rpb * nblk)
    if pad:
        t = torch.cat([t, t.new_zeros(B, pad, *t.shape[2:])], 1)
    t = t.reshape(B, -1, nblk, rpb, *t.shape[2:])
    acc = torch.zeros_like(t[:, 0])
    for p in range(t.shape[1]):
        acc = acc + t[:, p]
    return _run(acc.movedim(2, 0))


def frm_bwd(dout, x, cw, sw, h, w2, order="pair", V=None):
    """-> dx (2, B, N, C), dh (B, N, C), dcw (B, 2C), dw2 (2, C), db2 (2).  order "lanes" (fp32 only) is the
    kernel's own: lane-owned chunks folded by halves for the sums over C, per-block partials for the sums over
    rows, the blocks' partials added in fp64 as the test adds them"""
    C = x.shape[-1]
    if order == "lanes":
        return _frm_bwd_lanes(dout, x, cw, sw, h, w2, V)
    d1, d2, x1, x2 = dout[0], dout[1], x[0], x[1]
    c0, c1 = 0.5 * cw[:, None, :C], 0.5 * cw[:, None, C:]
    sw0, sw1 = sw[..., 0], sw[..., 1]
    dx = torch.stack([d1 + (c0 + 0.5 * sw0[..., None]) * d2, d2 + (c1 + 0.5 * sw1[..., None]) * d1])
    q1, q0 = d1 * x2, d2 * x1
    g0 = 0.5 * _sum(q0, -1, order) * sw0 * (1.0 - sw0)
    g1 = 0.5 * _sum(q1, -1, order) * sw1 * (1.0 - sw1)
    pos = h > 0
    zero = torch.zeros_like(h)
    dh = torch.where(pos, g0[..., None] * w2[0] + g1[..., None] * w2[1], zero)
    r = torch.where(pos, h, zero)
    dcw = 0.5 * torch.cat([_sum(q0, 1, order), _sum(q1, 1, order)], -1)
    dw2 = torch.stack([_sum((g0[..., None] * r).reshape(-1, C), 0, order), _sum((g1[..., None] * r).reshape(-1, C), 0, order)])
    db2 = torch.stack([_sum(g0.reshape(-1), 0, order), _sum(g1.reshape(-1), 0, order)])
    return dx, dh, dcw, dw2, db2


def _frm_bwd_lanes(dout, x, cw, sw, h, w2, V):
    C = x.shape[-1]
    d1, d2, x1, x2 = dout[0], dout[1], x[0], x[1]
    c0, c1 = 0.5 * cw[:, None, :C], 0.5 * cw[:, None, C:]
    sw0, sw1 = sw[..., 0], sw[..., 1]
    dx = torch.stack([d1 + (c0 + 0.5 * sw0[..., None]) * d2, d2 + (c1 + 0.5 * sw1[..., None]) * d1])
    q1, q0 = d1 * x2, d2 * x1
    g0 = 0.5 * _lane_rowsum(q0, V) * sw0 * (1.0 - sw0)
    g1 = 0.5 * _lane_rowsum(q1, V) * sw1 * (1.0 - sw1)
    pos = h > 0
    zero = torch.zeros_like(h)
    dh = torch.where(pos, g0[..., None] * w2[0] + g1[..., None] * w2[1], zero)
    r = torch.where(pos, h, zero)
    blocks = lambda t: _block_partials(t, C, V).double()
    dcw = torch.cat([(0.5 * blocks(q0)).sum(1), (0.5 * blocks(q1)).sum(1)], -1)
    dw2 = torch.stack([blocks(g0[..., None] * r).sum((0, 1)), blocks(g1[..., None] * r).sum((0, 1))])
    db2 = torch.stack([blocks(g0).sum(), blocks(g1).sum()])
    return dx, dh, dcw, dw2, db2


BWD_ORDERS = ORDERS + ("lanes",)
FRM_FWD_OUT = ("sw", "out")
FRM_BWD_OUT = ("dx", "dh", "dcw", "dw2", "db2")
ROWWISE = ("sw", "out", "dx", "dh", "y")


@functools.lru_cache(maxsize=None)
def frm_inputs(case, kind):
    """fp64 tensors exact in their storage type: x, h, dout in case.dtype; cw, w2, b2, sw fp32"""
    g = gen(case.name, kind)
    B, N, C, dt = case.B, case.N, case.C, case.dtype
    if kind == "gauss":
        x = randn(g, 2, B, N, C).to(dt).double()
        h = randn(g, B, N, C).to(dt).double()
        dout = randn(g, 2, B, N, C).to(dt).double()
        cw = torch.sigmoid(randn(g, B, 2 * C)).float().double()
        w2 = (randn(g, 2, C) * (2.0 / C ** 0.5)).float().double()
        b2 = (0.25 * randn(g, 2)).float().double()
        sw = torch.sigmoid(randn(g, B, N, 2)).float().double()
    else:
        x, dout = ints(g, -4, 4, 2, B, N, C), ints(g, -4, 4, 2, B, N, C)
        cw = pick(g, (0.0, 0.5, 1.0), B, 2 * C)
        w2 = ints(g, -2, 2, 2, C)
        b2 = torch.zeros(2, dtype=torch.float64)
        sw = pick(g, (0.0, 0.25, 0.5, 0.75, 1.0), B, N, 2)
        if kind == "exact":                       # h <= 0 (forward: sw == 0.5), with -0.0 among the zeros
            h = -ints(g, 0, 4, B, N, C)
        else:                                      # "pos": h > 0 everywhere and w2 = 0
            h = ints(g, 1, 4, B, N, C)
            w2 = torch.zeros(2, C, dtype=torch.float64)
    return dict(x=x, cw=cw, h=h, w2=w2, b2=b2, sw=sw, dout=dout)


def frm_bwd_h(case, kind):
    """the backward's exact kind runs on h of both signs with +0.0 and -0.0 present"""
    inp = frm_inputs(case, kind)
    if kind == "gauss":
        return inp["h"]
    g = gen(case.name, kind, "bwd_h")
    h = ints(g, -4, 4, case.B, case.N, case.C)
    neg = torch.randint(0, 2, h.shape, generator=g).bool() & (h == 0)
    return torch.where(neg, -torch.zeros_like(h), h)


@functools.lru_cache(maxsize=None)
def frm_expected(case, kind):
    """{name: fp64 reference}, {name: E_emul} (empty for the exact kinds)"""
    inp = frm_inputs(case, kind)
    hb = frm_bwd_h(case, kind)
    fwd = lambda p, **kw: frm_fwd(work(inp["x"], p), work(inp["cw"], p), work(inp["h"], p), work(inp["w2"], p),
                                  work(inp["b2"], p), **kw)
    bwd = lambda p, **kw: frm_bwd(work(inp["dout"], p), work(inp["x"], p), work(inp["cw"], p), work(inp["sw"], p),
                                  work(hb, p), work(inp["w2"], p), **kw)
    ref = dict(zip(FRM_FWD_OUT, fwd(torch.float64)))
    if case.bwd:
        ref.update(zip(FRM_BWD_OUT, bwd(torch.float64)))
    e = {}
    if kind == "gauss":
        for order in BWD_ORDERS if case.bwd else ORDERS:
            got = dict(zip(FRM_BWD_OUT, bwd(FP32, order=order, V=case.V))) if case.bwd else {}
            if order == "lanes":                   # a freedom of the backward's reductions alone
                for n, v in got.items():
                    if n in ("dx", "dh"):
                        v = v.to(case.dtype)
                    e[n] = max(e.get(n, 0.0), rowerr(v, ref[n]) if n in ROWWISE else tenerr(v, ref[n]))
                continue
            for form in FORMS:
                got.update(zip(FRM_FWD_OUT, fwd(FP32, order=order, form=form)))
                for n, v in got.items():
                    if n in ("out", "dx", "dh"):
                        v = v.to(case.dtype)
                    e[n] = max(e.get(n, 0.0), rowerr(v, ref[n]) if n in ROWWISE else tenerr(v, ref[n]))
    return ref, e


def out_ulp(name, dtype):
    return ULP[dtype] if name in ("out", "dx", "dh", "dsw", "da", "ctxT") else ULP32


def abs_sums_exact(terms, dim, unit):
    """every partial sum of `terms` along dim, in any order, is an integer multiple of `unit` below 2^24 units"""
    t = terms / unit
    return bool(torch.equal(t, t.round()) and (t.abs().sum(dim) < 2 ** 24).all())


# dout2: the kernel rounds dout + dout2 to T once.  Pairs whose sum is not representable, ties included:
# bf16 has 8 significant bits (256 + 1 is a tie, 256 + 3 too, 258 + 1 rounds to even), fp16 has 11
DOUT2_PAIRS = {
    BF16: ((256.0, 1.0), (256.0, 3.0), (258.0, 1.0), (256.0, 1.5), (256.0, -0.5), (-256.0, -1.0), (512.0, 2.0),
           (1.0, 2.0 ** -9), (1.0, 2.0 ** -8), (3.0, 1.0)),
    FP16: ((2048.0, 1.0), (2048.0, 3.0), (2050.0, 1.0), (2048.0, 1.5), (2048.0, -0.5), (-2048.0, -1.0), (4096.0, 2.0),
           (1.0, 2.0 ** -12), (1.0, 2.0 ** -11), (3.0, 1.0)),
    FP32: ((256.0, 1.0), (3.0, 1.0), (2.0 ** 24, 1.0), (2.0 ** 24, 3.0), (1.0, 2.0 ** -24), (-5.0, 0.25)),
}


def dout2_tensors(dtype, shape, g):
    """dout, dout2 in `dtype` drawn from DOUT2_PAIRS (either order), and their sum formed in `dtype`"""
    pairs = torch.tensor(DOUT2_PAIRS[dtype], dtype=torch.float64)
    idx = torch.randint(0, len(pairs), shape, generator=g)
    flip = torch.randint(0, 2, shape, generator=g).bool()
    a, b = pairs[idx, 0], pairs[idx, 1]
    d, d2 = torch.where(flip, b, a).to(dtype), torch.where(flip, a, b).to(dtype)
    assert torch.equal(d.double() + d2.double(), a + b)          # the pairs themselves are exact in dtype
    return d, d2, (d + d2)


# =========================================================== pooling backward
@dataclass(frozen=True, eq=False)
class PoolBwdCase:
    name: str
    dtype: torch.dtype
    C: int
    B: int
    N: int
    nslice: int
    kind: str
    aim: str = ""

    @property
    def wraps(self):
        return -(-self.N // rpb_of(self.C, vec_width(self.dtype))) > -(-512 // (2 * self.B))


def _pool_bwd_cases():
    out = []
    for dt in DTYPES:
        cs = (4, 160, 512) if dt == FP32 else (8, 160, 512, 1024)
        for i, C in enumerate(cs):
            ns = (1, 5, 16)[i % 3]
            out.append(PoolBwdCase(f"{name_of(dt)}_C{C}_B3_N67_s{ns}", dt, C, 3, 67, ns, "gauss"))
            out.append(PoolBwdCase(f"{name_of(dt)}_C{C}_B1_N64_s{(1, 5, 16)[(i + 1) % 3]}_exact", dt, C, 1, 64,
                                   (1, 5, 16)[(i + 1) % 3], "exact"))
    out.append(PoolBwdCase("wrap_bf16_C512_B8_N133", BF16, 512, 8, 133, 16, "gauss", "wraps the grid at B = 8"))
    out.append(PoolBwdCase("wrap_bf16_C512_B1_N1031", BF16, 512, 1, 1031, 5, "gauss", "wraps the grid at B = 1"))
    out.append(PoolBwdCase("wrap_fp32_C4_B1_N32768", FP32, 4, 1, 32768, 1, "exact", "wraps the grid at B = 1, TPR = 4"))
    return out


POOL_BWD_CASES = _pool_bwd_cases()
NO_ARGMAX = 0x7FFFFFFF


@functools.lru_cache(maxsize=None)
def pool_bwd_inputs(case):
    """part (nslice, B, 4C) fp32, argmax (B, 2C) int32 (token 0, N - 1, interior; one channel NO_ARGMAX), dx0"""
    g = gen(case.name)
    B, N, C, dt = case.B, case.N, case.C, case.dtype
    if case.kind == "exact":                       # integer slices, N a power of two: sum / N is a multiple of 1/4
        part = ints(g, -1, 1, case.nslice, B, 4 * C)
        part[:, :, :2 * C] *= N / 4
        dx0 = ints(g, -4, 4, 2, B, N, C)
    else:
        part = randn(g, case.nslice, B, 4 * C).float().double()
        dx0 = randn(g, 2, B, N, C).to(dt).double()
    am = torch.randint(0, N, (B, 2 * C), generator=g, dtype=torch.int32)
    am[:, 0::3] = 0
    am[:, 1::3] = N - 1
    am[B - 1, 2 * C - 1] = NO_ARGMAX
    am[0, C // 2] = NO_ARGMAX
    return part, am, dx0


def pool_bwd_formula(part, am, dx0, order="pair"):
    """dx (2, B, N, C) = dx0 + (avg / N + [n == argmax] max)"""
    _, B, N, C = dx0.shape
    t = _sum(part, 0, order)                                       # (B, 4C)
    avg = (t[:, :2 * C] / N).view(B, 2, C).transpose(0, 1)         # (g, B, C)
    mx = t[:, 2 * C:].view(B, 2, C).transpose(0, 1)
    hit = torch.arange(N).view(1, 1, N, 1) == am.view(B, 2, 1, C).transpose(0, 1).long()
    return dx0 + (avg[:, :, None, :] + torch.where(hit, mx[:, :, None, :], torch.zeros_like(mx[:, :, None, :])))


@functools.lru_cache(maxsize=None)
def pool_bwd_expected(case):
    part, am, dx0 = pool_bwd_inputs(case)
    ref = pool_bwd_formula(part, am, dx0)
    e = 0.0
    if case.kind == "gauss":
        for order in ORDERS:
            e = max(e, rowerr(pool_bwd_formula(part.float(), am, dx0.float(), order).to(case.dtype), ref))
    return ref, e


# =========================================================== the channel-MLP GEMV pair
ACT = {"none": 0, "relu": 2, "sigmoid": 3}


def _dot(x, w, order):
    """x (M, K) w (Nout, K) -> (M, Nout); seq: four columns at a time, in order (the kernel's float4 steps)"""
    if order == "pair" or x.dtype == torch.float64:
        return x @ w.t()
    acc = torch.zeros(x.shape[0], w.shape[0], dtype=x.dtype)
    for k in range(0, x.shape[1], 4):
        acc = acc + x[:, k:k + 4] @ w[:, k:k + 4].t()
    return acc


def act_fwd(z, act, form="exp"):
    if act == "relu":
        return torch.where(z > 0, z, torch.zeros_like(z))
    return sigmoid(z, form) if act == "sigmoid" else z


def linear_fwd(x, w, b, act, order="pair", form="exp"):
    z = _dot(x, w, order)
    return act_fwd(z + b if b is not None else z, act, form)


@dataclass(frozen=True, eq=False)
class LinFwdCase:
    M: int
    K: int
    Nout: int
    act: str
    bias: bool
    kind: str
    aim: str = ""

    @property
    def name(self):
        return f"M{self.M}_K{self.K}_N{self.Nout}_{self.act}_{'b' if self.bias else 'nob'}_{self.kind}"


LIN_FWD_CASES = [
    LinFwdCase(1, 4, 1, "none", True, "gauss", "one float4, one live wave"),
    LinFwdCase(1, 4, 1, "relu", False, "exact"),
    LinFwdCase(3, 128, 5, "sigmoid", True, "gauss", "a block with three idle waves"),
    LinFwdCase(3, 128, 5, "relu", True, "exact"),
    LinFwdCase(8, 1028, 5, "none", False, "gauss", "the four-loads loop and a one-lane tail; b = NULL"),
    LinFwdCase(8, 1028, 5, "none", True, "exact"),
    LinFwdCase(8, 1028, 1, "relu", True, "gauss"),
    LinFwdCase(8, 2048, 5, "sigmoid", False, "gauss", "exactly 64 KiB of dynamic LDS"),
    LinFwdCase(8, 2048, 4096, "relu", True, "exact", "64 KiB of LDS, 1024 blocks"),
    LinFwdCase(3, 2048, 4096, "none", True, "gauss"),
    LinFwdCase(1, 128, 4096, "sigmoid", True, "gauss"),
    LinFwdCase(3, 4, 5, "sigmoid", False, "exact", "w = 0, b = NULL: sigmoid(0) == 0.5"),
]


@functools.lru_cache(maxsize=None)
def lin_fwd_inputs(case):
    g = gen("linfwd", case.name)
    M, K, Nout = case.M, case.K, case.Nout
    if case.kind == "exact":
        x, w = ints(g, -3, 3, M, K), ints(g, -2, 2, Nout, K)
        if case.act == "sigmoid":
            w = torch.zeros_like(w)
        b = ints(g, -8, 8, Nout) if case.bias else None
    else:
        x = randn(g, M, K).float().double()
        w = (randn(g, Nout, K) / K ** 0.5).float().double()
        b = (0.5 * randn(g, Nout)).float().double() if case.bias else None
    return x, w, b


@functools.lru_cache(maxsize=None)
def lin_fwd_expected(case):
    x, w, b = lin_fwd_inputs(case)
    ref = linear_fwd(x, w, b, case.act)
    e = 0.0
    if case.kind == "gauss":
        for order in ORDERS:
            for form in FORMS if case.act == "sigmoid" else FORMS[:1]:
                e = max(e, tenerr(linear_fwd(x.float(), w.float(), work(b, FP32), case.act, order, form), ref))
    return ref, e


NSLICE, SLICE_MAX = 16, 256


def linear_bwd(part, y, x, w, act, order="pair"):
    """part (nsl, M, Nout) -> dz, dx (M, K), dw (Nout, K), db (Nout)"""
    dy = _sum(part, 0, order)
    if act == "relu":
        dz = torch.where(y > 0, dy, torch.zeros_like(dy))
    elif act == "sigmoid":
        dz = dy * (y * (1.0 - y))
    else:
        dz = dy
    if order == "pair":
        return dz, dz @ w, dz.t() @ x, dz.sum(0)
    dx = torch.zeros(dz.shape[0], w.shape[1], dtype=dz.dtype)     # seq: sixteen output features at a time, in order
    for n in range(0, w.shape[0], 16):
        dx = dx + dz[:, n:n + 16] @ w[n:n + 16]
    dw = torch.zeros_like(w)
    for m in range(dz.shape[0]):                                   # and the rows one after the other
        dw = dw + dz[m][:, None] * x[m][None, :]
    return dz, dx, dw, _sum(dz, 0, order)


@dataclass(frozen=True, eq=False)
class LinBwdCase:
    K: int
    Nout: int
    nslice: int
    act: str
    accumulate: int
    kind: str
    db: bool = True
    dxp: bool = True
    M: int = 8

    @property
    def name(self):
        return (f"K{self.K}_N{self.Nout}_s{self.nslice}_{self.act}_acc{self.accumulate}_{self.kind}"
                f"{'' if self.db else '_nodb'}{'' if self.dxp else '_nodx'}")


LIN_BWD_CASES = [
    LinBwdCase(1, 10, 1, "none", 0, "exact"),
    LinBwdCase(63, 10, 2, "relu", 1, "exact"),
    LinBwdCase(65, 10, 7, "sigmoid", 0, "gauss"),
    LinBwdCase(65, 10, 75, "relu", 1, "gauss"),
    LinBwdCase(63, 10, 256, "none", 0, "gauss", db=False),
    LinBwdCase(65, 10, 7, "relu", 0, "exact", dxp=False),
    LinBwdCase(2048, 10, 2, "sigmoid", 1, "gauss"),
    LinBwdCase(1, 4096, 7, "relu", 0, "gauss"),
    LinBwdCase(65, 4096, 256, "sigmoid", 0, "gauss"),
    LinBwdCase(63, 4096, 75, "none", 1, "exact"),
    LinBwdCase(2048, 4096, 2, "relu", 0, "exact"),
    LinBwdCase(2048, 4096, 1, "sigmoid", 1, "gauss", db=False),
]


@functools.lru_cache(maxsize=None)
def lin_bwd_inputs(case):
    """part (nslice, M, Nout), y (M, Nout) the saved output, x (M, K), w (Nout, K), dw0 (Nout, K), db0 (Nout)"""
    g = gen("linbwd", case.name)
    M, K, Nout, ns = case.M, case.K, case.Nout, case.nslice
    if case.kind == "exact":
        part = ints(g, -1, 1, ns, M, Nout) * (torch.rand(ns, 1, 1, generator=g, dtype=torch.float64) < 8.0 / ns)
        x, w = ints(g, -3, 3, M, K), ints(g, -2, 2, Nout, K)
        dw0, db0 = ints(g, -8, 8, Nout, K), ints(g, -8, 8, Nout)
        y = ints(g, 0, 3, M, Nout) if case.act != "sigmoid" else pick(g, (0.5,), M, Nout)
    else:
        part = (randn(g, ns, M, Nout) / ns ** 0.5).float().double()
        x = randn(g, M, K).float().double()
        w = (randn(g, Nout, K) / K ** 0.5).float().double()
        dw0, db0 = randn(g, Nout, K).float().double(), randn(g, Nout).float().double()
        if case.act == "sigmoid":
            y = torch.sigmoid(randn(g, M, Nout)).float().double()
        else:                                      # relu: saved outputs, exactly 0 on about half
            y = randn(g, M, Nout).clamp_min(0.0).float().double()
    return part, y, x, w, dw0, db0


@functools.lru_cache(maxsize=None)
def lin_bwd_expected(case):
    """fp64 (dx, dw, db) with the accumulate pre-fill added, and E_emul per tensor"""
    part, y, x, w, dw0, db0 = lin_bwd_inputs(case)
    acc = case.accumulate

    def run(p, order):
        _, dx, dw, db = linear_bwd(work(part, p), work(y, p), work(x, p), work(w, p), case.act, order)
        return dx, (dw + work(dw0, p) if acc else dw), (db + work(db0, p) if acc else db)

    ref = run(torch.float64, "pair")
    e = [0.0, 0.0, 0.0]
    if case.kind == "gauss":
        for order in ORDERS:
            e = [max(a, tenerr(v, r)) for a, v, r in zip(e, run(FP32, order), ref)]
    return ref, e


# =========================================================== FFM context softmax
FFM_SHAPES = [(D, B, H) for D in (16, 32, 64) for B, H in ((1, 1), (3, 5), (1, 8), (3, 8))]
FFM_KINDS = ("gauss", "large", "const", "onehot")


def ffm_scale(D, kind):
    return 0.25 if kind == "large" else D ** -0.5


@functools.lru_cache(maxsize=None)
def ffm_fwd_inputs(D, B, H, kind):
    """kv (2, B, H, D, D) fp32, every (g, b, head) a matrix of its own"""
    g = gen("ffm", D, B, H, kind)
    shape = (2, B, H, D, D)
    if kind == "gauss":
        return (randn(g, *shape) * (ZMAX / 4 / ffm_scale(D, kind))).float().double()
    if kind == "large":
        # kv scale is an integer up to 1e4 in magnitude (scale = 1/4, kv a multiple of 4): the product and the
        # difference to the column's maximum are exact in fp32, fused or not; each column has entries within 6
        # of its maximum and entries thousands below
        top = ints(g, -10000, 9990, 2, B, H, 1, D)
        near = ints(g, -6, 0, *shape)
        far = ints(g, -9000, -100, *shape)
        z = top + torch.where(torch.rand(shape, generator=g) < 0.5, near, far)
        return z.clamp(-10000, 10000) * 4.0
    if kind == "const":
        return ints(g, -9, 9, 2, B, H, 1, D).expand(*shape).contiguous()
    assert kind == "onehot"
    kv = ints(g, -9, 9, 2, B, H, 1, D).expand(*shape).contiguous()
    hot = torch.randint(0, D, (2, B, H, 1, D), generator=g)
    return kv + 1000.0 / ffm_scale(D, "large") * (torch.arange(D).view(1, 1, 1, D, 1) == hot)


def ffm_fwd(kv, scale, order="pair", form="exp"):
    """softmax over dim -2 of kv scale (the maximum subtracted)"""
    v = kv * scale
    e = _exp(v - v.amax(-2, keepdim=True), form)
    return e * (1.0 / _sum(e, -2, order).unsqueeze(-2))


def ffm_bwd(ctx, dctx_swapped, scale, order="pair"):
    """ctx (2, B, H, D, D); dctx_swapped[g] = the gradient filed under 1 - g"""
    s = _sum(ctx * dctx_swapped, -2, order).unsqueeze(-2)
    return scale * ctx * (dctx_swapped - s)


@functools.lru_cache(maxsize=None)
def ffm_fwd_expected(D, B, H, kind, dtype):
    kv = ffm_fwd_inputs(D, B, H, kind)
    sc = ffm_scale(D, kind)
    if kind == "onehot":
        sc = ffm_scale(D, "large")
    sc32 = float(torch.tensor(sc, dtype=torch.float32))
    ref = ffm_fwd(kv, sc32)
    e = {"ctx": 0.0, "ctxT": 0.0}
    if kind in ("gauss", "large"):
        for order in ORDERS:
            for form in FORMS:
                got = ffm_fwd(kv.float(), sc32, order, form)
                e["ctx"] = max(e["ctx"], tenerr(got, ref))
                e["ctxT"] = max(e["ctxT"], tenerr(got.to(dtype), ref))
    return kv, sc32, ref, e


@functools.lru_cache(maxsize=None)
def ffm_bwd_expected(D, B, H, kind, dtype):
    """ctx, dctx (as filed: under the consumer), scale, the fp64 da, E_emul"""
    g = gen("ffmbwd", D, B, H, kind)
    shape = (2, B, H, D, D)
    if kind == "exact":
        ctx, dctx, sc = torch.full(shape, 1.0 / D, dtype=torch.float64), ints(g, -4, 4, *shape), 0.25
    else:
        ctx = torch.softmax(randn(g, *shape) * 2, -2).float().double()
        dctx, sc = randn(g, *shape).float().double(), float(torch.tensor(D ** -0.5, dtype=torch.float32))
    ref = ffm_bwd(ctx, dctx.flip(0), sc)
    e = 0.0
    if kind != "exact":
        for order in ORDERS:
            e = max(e, tenerr(ffm_bwd(ctx.float(), dctx.float().flip(0), sc, order).to(dtype), ref))
    return ctx, dctx, sc, ref, e


# =========================================================== row LayerNorm (fp32 rows of any width)
ROWLN_EPS = 1e-5
ROWLN_SHAPES = [(R, C) for R in (1, 3, 8) for C in (1, 64, 255, 257, 2048)]
ROWLN_KINDS = ("random", "offset", "const")


@functools.lru_cache(maxsize=None)
def rowln_inputs(R, C, kind):
    g = gen("rowln", R, C, kind)
    if kind == "random":
        x = (randn(g, R, C) * 2 + 0.5).float().double()
    elif kind == "offset":
        x = 64.0 + ints(g, -8, 8, R, C) * 0.125
    else:
        x = ints(g, -8, 8, R, 1).expand(R, C).contiguous()
    gamma = (1.0 + 0.5 * randn(g, C)).float().double()
    beta = randn(g, C).float().double()
    dy = ints(g, -4, 4, R, C)
    return x, gamma, beta, dy


def rowln_fwd(x, gamma, beta, eps, order="pair", one_pass=False):
    C = x.shape[1]
    mu = _sum(x, 1, order) / C
    if one_pass:
        q = (_sum(x * x, 1, order) / C - mu * mu).clamp_min(0.0)
    else:
        d = x - mu[:, None]
        q = _sum(d * d, 1, order) / C
    rs = torch.rsqrt(q + eps)
    return (x - mu[:, None]) * rs[:, None] * gamma + beta, mu, rs


def rowln_bwd(dy, x, gamma, mu, rs, order="pair"):
    C = x.shape[1]
    xh = (x - mu[:, None]) * rs[:, None]
    t = dy * gamma
    m1 = _sum(t, 1, order) / C
    m2 = _sum(t * xh, 1, order) / C
    dx = rs[:, None] * (t - m1[:, None] - xh * m2[:, None])
    return dx, _sum(dy * xh, 0, order), _sum(dy, 0, order)


ROWLN_OUT = ("y", "mean", "rstd", "dx", "dgamma", "dbeta")


@functools.lru_cache(maxsize=None)
def rowln_expected(R, C, kind):
    """the backward takes the saved statistics as inputs: the fp64 ones rounded to fp32"""
    x, gamma, beta, dy = rowln_inputs(R, C, kind)
    y, mu, rs = rowln_fwd(x, gamma, beta, ROWLN_EPS)
    mu32, rs32 = mu.float(), rs.float()
    ref = dict(zip(ROWLN_OUT, (y, mu, rs) + rowln_bwd(dy, x, gamma, mu32.double(), rs32.double())))
    e = {}
    eps32 = float(torch.tensor(ROWLN_EPS, dtype=torch.float32))
    for order in ORDERS:
        got = rowln_fwd(x.float(), gamma.float(), beta.float(), eps32, order) + \
            rowln_bwd(dy.float(), x.float(), gamma.float(), mu32, rs32, order)
        for n, v in zip(ROWLN_OUT, got):
            e[n] = max(e.get(n, 0.0), rowln_err(n, v, ref, R, C, kind))
    return ref, e, (mu32, rs32)


def rowln_err(name, got, ref, R, C, kind):
    """y per row; dx per row relative to max |rstd dy gamma|, the size of the terms its formula subtracts (at C = 1
    and on constant rows dx is a difference of equal terms: the reference is 0 or far below them, and a fused
    dy gamma - mean leaves one rounding of the product); the rest per tensor"""
    if name == "y":
        return rowerr(got, ref[name])
    if name == "dx":
        _, gamma, _, dy = rowln_inputs(R, C, kind)
        scale = (ref["rstd"][:, None] * dy * gamma).abs().amax(1).clamp_min(TINY)
        return ((got.detach().double().cpu() - ref[name]).abs().amax(1) / scale).max().item()
    return tenerr(got, ref[name])


# =========================================================== IFRM combine
IFRM_BN = ((1, 1), (3, 15), (1, 16), (1, 17), (3, 67))
IFRM_RUNS = [(dt, C, B, N, kind) for dt in DTYPES for C in (vec_width(dt), 32, 160, 320, 512) for B, N in IFRM_BN
             for kind in ("gauss", "exact")]


def ifrm_run_id(r):
    return f"{name_of(r[0])}_C{r[1]}_B{r[2]}_N{r[3]}_{r[4]}"


@functools.lru_cache(maxsize=None)
def ifrm_inputs(dt, C, B, N, kind):
    g = gen("ifrm", name_of(dt), C, B, N, kind)
    if kind == "gauss":
        x, dout = randn(g, 2, B, N, C).to(dt).double(), randn(g, 2, B, N, C).to(dt).double()
        cw = randn(g, B, 2 * C).float().double()
        sw = randn(g, B, N, 2).to(dt).double()
        lc, ls = (torch.tensor([v], dtype=torch.float64).float().double() for v in (0.37, -0.61))
    else:
        x, dout = ints(g, -4, 4, 2, B, N, C), ints(g, -4, 4, 2, B, N, C)
        cw = pick(g, (0.0, 0.5, 1.0, -0.25), B, 2 * C)
        sw = pick(g, (0.0, 0.5, -1.0, 0.25, 2.0), B, N, 2)
        lc, ls = torch.tensor([0.5], dtype=torch.float64), torch.tensor([-0.25], dtype=torch.float64)
    return dict(x=x, dout=dout, cw=cw, sw=sw, lc=lc, ls=ls)


def ifrm_fwd(x, cw, sw, lc, ls):
    C = x.shape[-1]
    k1 = lc * cw[:, None, C:] + ls * sw[..., 1:2]
    k0 = lc * cw[:, None, :C] + ls * sw[..., 0:1]
    return torch.stack([x[0] + k1 * x[1], x[1] + k0 * x[0]])


def ifrm_bwd(dout, x, cw, sw, lc, ls, order="pair"):
    """-> dx, dsw (B, N, 2), dcw (B, 2C), dlc, dls"""
    C = x.shape[-1]
    d1, d2, a, bb = dout[0], dout[1], x[0], x[1]
    k1 = lc * cw[:, None, C:] + ls * sw[..., 1:2]
    k0 = lc * cw[:, None, :C] + ls * sw[..., 0:1]
    dx = torch.stack([d1 + k0 * d2, d2 + k1 * d1])
    u1, u0 = d1 * bb, d2 * a
    r0, r1 = _sum(u0, -1, order), _sum(u1, -1, order)
    dsw = torch.stack([ls * r0, ls * r1], -1)
    t = torch.cat([_sum(u0, 1, order), _sum(u1, 1, order)], -1)          # (B, 2C)
    dcw = lc * t
    dlc = _sum((cw * t).reshape(-1), 0, order)
    dls = _sum((sw[..., 0] * r0 + sw[..., 1] * r1).reshape(-1), 0, order)
    return dx, dsw, dcw, dlc, dls


IFRM_OUT = ("out", "dx", "dsw", "dcw", "dlc", "dls")


@functools.lru_cache(maxsize=None)
def ifrm_expected(dt, C, B, N, kind):
    inp = ifrm_inputs(dt, C, B, N, kind)
    run = lambda p, **kw: (ifrm_fwd(*(work(inp[k], p) for k in ("x", "cw", "sw", "lc", "ls"))),) + \
        ifrm_bwd(*(work(inp[k], p) for k in ("dout", "x", "cw", "sw", "lc", "ls")), **kw)
    ref = dict(zip(IFRM_OUT, run(torch.float64)))
    e = {}
    if kind == "gauss":
        for order in ORDERS:
            for n, v in zip(IFRM_OUT, run(FP32, order=order)):
                if n in ("out", "dx", "dsw"):
                    v = v.to(dt)
                e[n] = max(e.get(n, 0.0), rowerr(v, ref[n]) if n in ROWWISE else tenerr(v, ref[n]))
    return ref, e


# =========================================================== the record the GPU tests print
def report(test, case, tensor, err=None, bnd=None, exact=None):
    """one line per check: a ratio for a bounded check, the word for an exact one"""
    if exact is not None:
        print(f"[rectify] {test} {case} | {tensor} exact {bool(exact)}")
    else:
        print(f"[rectify] {test} {case} | {tensor} err {err:.3e} bound {bnd:.3e} ratio {err / bnd:.3f}")
