"""The exact-result cases of the MFMA GEMM family: one table, read by tests/test_gemm_variants.py
(CPU: csrc/gemm_plan.h gives every case exactly the kernel variant it names) and by
tests/test_gpu_gemm_exact.py (GPU: that variant computes the case exactly).

Inputs for which the GEMM is exact.  A and B hold values of {-2, -1, 1, 2}: exact in bf16, fp16
and fp32, every product an integer, every partial sum in any order (MFMA lanes, k-group waves,
split-K slabs, the streaming ring) an integer below 4 K <= 2^17 for K <= 16392, so the fp32
accumulator is exact whatever the summation order.  The epilogue is exact too: bias in multiples
of 1/4 in [-4, 4], residual / accumulate target small integers, rscale of {0, 0.5, 1, 1.25} (the
pre-activation is a multiple of 1/4 below 2^18, 1.25 x it a multiple of 1/16: 22 bits), and
rows_per_sample = 37, which divides no tile height.  What is left is the rounding of a 16-bit
store, which the kernels do with the hardware round-to-nearest-even convert: the expected value is
`ref.float().to(dtype)`, and sums above 256 (bf16) / 2048 (fp16) also check the tie rule.  GELU is
the one inexact epilogue (gelu_delta below).

Guards.  C (and R, the mask) is a column slice of a wider buffer (ldc > N) with guard rows after
row M, all filled with a sentinel that must survive; A and B are views of buffers with
ld = K + 8 (transposed operands: ld = rows + 8) and guard rows whose padding is NaN, so a read
past K or past the last row of a group poisons the result instead of being multiplied in."""
from __future__ import annotations

from collections import namedtuple
from dataclasses import dataclass, field

PATH_GENERIC, PATH_TILE, PATH_STREAM = 0, 1, 2
NUM_CU = 256                      # the CU count the plans are pinned at (MI355X)
RPS = 37                          # rows per DropPath sample: divides neither 64 nor 128
GUARD_ROWS = 8
SENTINEL = -3072.0                # exact in bf16 / fp16 / fp32, outside every stored range checked
KNOB_DEFAULTS = dict(GEMM_TILES=1, GEMM_SMALLK=256, GEMM_T128=400, GEMM_SPLITKW=1, GEMM_KW=2, GEMM_MID=50,
                     GEMM_STREAM=1024, GEMM_STREAM_K=128, GEMM_STREAM_BPC=4, GROUPED_KT=48)

# the kernel a case must run: path, tile, LDS ring slots, k-group waves, whether split-K slabs
# are written, and the reducer's z-lanes (0 = no reducer)
Variant = namedtuple("Variant", "path bm bn ns kw split red_zl")


def tile(bm, bn, ns, kw=1, red_zl=0):
    return Variant(PATH_TILE, bm, bn, ns, kw, red_zl > 0, red_zl)


STREAM = Variant(PATH_STREAM, 64, 64, 0, 1, False, 0)


def generic(bm, bn, red_zl=0):
    return Variant(PATH_GENERIC, bm, bn, 0, 1, red_zl > 0, red_zl)


# ---------------------------------------------------------------------------------- epilogues
# bias: True, or "strided" (a (G, N) view of a wider buffer: per-group bias stride);
# res: True, or "inplace" (R = C itself, as the FFM's ReLU backward uses the mask epilogue)
EPIS = {
    "plain": {},
    "combo": dict(bias=True, act="relu", res=True, rscale=True, mask=True),
    "relu": dict(bias=True, act="relu"),
    "gelu": dict(bias=True, act="gelu"),
    "res": dict(bias=True, res=True),
    "res_scale": dict(bias=True, res=True, rscale=True),
    "mask": dict(bias=True, mask=True),
    "mask_res": dict(res="inplace", mask=True),
    "fp32": dict(bias=True, out_mode=1),
    "acc": dict(out_mode=2),
    "a2": dict(bias=True, a2=True),
    "g2bias": dict(bias="strided", act="relu", res=True, rscale=True),
    "dbias": dict(out_mode=1, dbias=True),
    "dbias_acc": dict(out_mode=2, dbias=True),
}
BASIC = ("plain", "combo")
FULL = ("plain", "combo", "relu", "gelu", "res", "res_scale", "mask", "mask_res", "fp32", "acc", "a2")


@dataclass(frozen=True)
class Case:
    name: str
    G: int
    M: int
    N: int
    K: int
    variant: Variant
    epis: tuple = BASIC
    tA: int = 0
    tB: int = 0
    knobs: dict = field(default_factory=dict)
    splitk: int = 0               # requested split, 0 = the library's choice
    cvec: bool = True             # ldc keeps C's rows 16-B aligned (the vector epilogue)
    dtypes: tuple = ("bfloat16", "float16")
    fast: int = 1                 # operands eligible for the LDS-DMA path
    cu: bool = False              # the plan depends on the CU count
    other: dict = field(default_factory=dict)   # epilogue -> another variant (e.g. A2 leaves the stream path)


T = tile
C128 = dict(GEMM_T128=0)
CASES = [
    # ---- 64 x 64 tiles
    Case("t64_ns4_kw1", 1, 100, 72, 72, T(64, 64, 4), FULL),
    Case("t64_ns4_kw1_g2", 2, 100, 72, 72, T(64, 64, 4), ("g2bias",)),
    Case("t64_ns4_kw1_scalar", 1, 100, 72, 72, T(64, 64, 4), ("plain", "combo", "gelu"), cvec=False),
    Case("t64_ns4_kw1_tB", 1, 100, 72, 72, T(64, 64, 4), tB=1),
    Case("t64_ns4_kw1_tAtB", 1, 104, 72, 72, T(64, 64, 4), tA=1, tB=1),
    Case("t64_ns4_kw1_tA", 1, 104, 72, 72, T(64, 64, 4), tA=1),
    Case("t64_ns4_kw1_tiny", 1, 5, 3, 8, T(64, 64, 4)),
    Case("t64_ns4_kw2", 1, 100, 72, 264, T(64, 64, 4, 2), BASIC + ("a2",)),
    Case("t64_ns4_kw2_tB", 1, 100, 72, 264, T(64, 64, 4, 2), tB=1),
    Case("t64_ns4_kw2_tAtB", 1, 104, 72, 261, T(64, 64, 4, 2), tA=1, tB=1),
    Case("t64_ns2_kw2", 1, 1300, 1300, 264, T(64, 64, 2, 2)),
    Case("t64_ns2_kw1", 1, 2000, 1100, 72, T(64, 64, 2)),
    Case("t64_ns2_kw4", 1, 100, 72, 1032, T(64, 64, 2, 4), BASIC + ("a2",), knobs=dict(GEMM_KW=4)),
    Case("t64_ns2_kw4_tA", 1, 104, 72, 1032, T(64, 64, 2, 4), tA=1, knobs=dict(GEMM_KW=4)),
    # ---- 64 x 128 (the MID rule)
    Case("t64x128_ns2", 1, 2400, 2200, 72, T(64, 128, 2), FULL, cu=True),
    Case("t64x128_ns2_tB", 1, 2400, 2200, 72, T(64, 128, 2), tB=1, cu=True),
    Case("t64x128_ns2_tAtB", 1, 2400, 2200, 72, T(64, 128, 2), tA=1, tB=1, cu=True),
    Case("t64x128_ns2_g2", 2, 1300, 2200, 72, T(64, 128, 2), ("g2bias",), cu=True),
    # ---- 128 x 64
    Case("t128x64_ns2", 2, 25700, 40, 72, T(128, 64, 2), knobs=dict(GEMM_SMALLK=0)),
    Case("t128x64_ns4", 1, 300, 40, 72, T(128, 64, 4), knobs=dict(GEMM_SMALLK=0, GEMM_T128=0)),
    Case("t128x64_ns4_tAtB", 1, 304, 40, 72, T(128, 64, 4), tA=1, tB=1, knobs=dict(GEMM_SMALLK=0, GEMM_T128=0)),
    # ---- 128 x 128
    Case("t128_ns2", 1, 2600, 2600, 264, T(128, 128, 2), FULL),
    Case("t128_ns2_g2", 2, 1300, 2600, 264, T(128, 128, 2), ("g2bias",)),
    Case("t128_ns2_tB", 1, 2600, 2600, 264, T(128, 128, 2), tB=1),
    Case("t128_ns2_tAtB", 1, 2600, 2600, 261, T(128, 128, 2), tA=1, tB=1),
    Case("t128_ns2_tA", 1, 2600, 2600, 264, T(128, 128, 2), tA=1),
    Case("t128_ns4", 1, 300, 300, 520, T(128, 128, 4), knobs=C128, splitk=1),
    Case("t128_ns4_red_zl1", 1, 300, 300, 520, T(128, 128, 4, 1, 1), knobs=C128),
    # ---- the streaming grid (an A2 problem is not eligible and takes one block per tile)
    Case("stream", 1, 8200, 520, 72, STREAM, FULL, cu=True, other={"a2": T(64, 64, 2)}),
    Case("stream_tB", 1, 8200, 520, 72, STREAM, tB=1, cu=True),
    Case("stream_g2", 2, 8200, 520, 72, STREAM, ("g2bias",), cu=True),
    Case("stream_n40", 1, 65700, 40, 72, STREAM, cu=True),
    # ---- split-K: 64 x 64 NS4 slabs + the reducer, whose epilogue this is
    Case("red_zl1", 1, 100, 72, 2120, T(64, 64, 4, 1, 1), FULL),                 # nsplit 7, vector columns
    Case("red_zl1_g2", 2, 100, 72, 2120, T(64, 64, 4, 1, 1), ("g2bias",)),
    Case("red_zl4", 1, 100, 76, 4104, T(64, 64, 4, 1, 4), FULL),                 # nsplit 13, nv = 4 tail group
    Case("red_zl4_g2", 2, 100, 76, 4104, T(64, 64, 4, 1, 4), ("g2bias",)),
    Case("red_zl16_scalar", 1, 100, 75, 16392, T(64, 64, 4, 1, 16), FULL, cvec=False),   # nsplit 52, scalar columns
    Case("red_zl16_g2", 2, 50, 75, 16392, T(64, 64, 4, 1, 16), ("g2bias",), cvec=False),
    Case("red_tAtB_k2101", 1, 104, 72, 2101, T(64, 64, 4, 1, 1), ("plain", "combo", "fp32"), tA=1, tB=1),
    Case("red_dbias", 1, 72, 104, 2101, T(64, 64, 4, 1, 1), ("dbias", "dbias_acc"), tA=1, tB=1),
    # ---- the register-staged generic path: fp32, and 16-bit operands with K = 9 (ld = 17)
    Case("generic_f32", 1, 100, 72, 72, generic(128, 128), ("plain", "combo", "gelu", "fp32", "acc", "a2"),
         dtypes=("float32",), fast=0),
    Case("generic_f32_tB", 1, 100, 72, 72, generic(128, 128), tB=1, dtypes=("float32",), fast=0),
    Case("generic_f32_red", 1, 100, 72, 2120, generic(128, 128, 4), dtypes=("float32",), fast=0),
    Case("generic_h16_k9", 1, 100, 75, 9, generic(128, 128), cvec=False, fast=0),
]

# cmx_gemm_ln: the only launch that reaches 64 x 128 NS4 (one tile spans the row); the stored C is
# checked exactly, the normalised output stays with test_gemm_ln_tail
LN_CASE = Case("ln_t64x128_ns4", 1, 130, 128, 64, T(64, 128, 4), ("res_scale",))

# multi launches: problems (G, M, N, K, epilogue) of one cmx_gemm_multi grid, and the (NS, KW) the
# combined grid and the shortest k-loop give
MultiCase = namedtuple("MultiCase", "name tB problems ns kw")
MULTI_CASES = [
    MultiCase("multi_ns4_kw1", 0, ((1, 100, 72, 72, "relu"), (1, 130, 40, 72, "plain"), (2, 70, 136, 136, "g2bias")), 4, 1),
    MultiCase("multi_ns4_kw2", 1, ((1, 100, 72, 264, "plain"), (1, 130, 40, 328, "res_scale")), 4, 2),
    MultiCase("multi_ns2_kw2", 1, ((1, 1300, 520, 264, "plain"), (1, 1000, 264, 264, "combo")), 2, 2),
    MultiCase("multi_ns2_kw1", 0, ((1, 2000, 1100, 72, "relu"), (1, 100, 72, 72, "combo")), 2, 1),
]

Run = namedtuple("Run", "case epi dtype variant")


def runs(cases=None):
    """every (case, epilogue, dtype) that is run, with the variant it must take"""
    out = []
    for c in CASES if cases is None else cases:
        for dt in c.dtypes:
            for e in c.epis:
                out.append(Run(c, e, dt, c.other.get(e, c.variant)))
    return out


def run_id(r):
    return f"{r.case.name}-{r.epi}-{r.dtype}"


DTYPE_CODE = {"float32": 0, "bfloat16": 1, "float16": 2}


def plan_row(kind, G, M, N, K, tA=0, tB=0, ones=0, dtype=1, fast=1, splitk=0, a2=0, row_ln=0, tile_only=0, knobs=None):
    """one input line of tests/host/gemm_plan_dump.cpp"""
    k = dict(KNOB_DEFAULTS, **(knobs or {}))
    cols = [kind, G, M, N, K, tA, tB, ones, dtype, fast, splitk, a2, row_ln, 0, 0, 0, 1, tile_only] + \
           [k[n] for n in KNOB_DEFAULTS] + [NUM_CU]
    return "\t".join(str(c) for c in cols)


# ------------------------------------------------------------------------------------- GELU
# The kernels' GELU is y = 0.5f * v * (1.f + cmx_erf(v * 0.70710678f)) in fp32 on the exact
# pre-activation v.  Against fp64 erf-GELU of v:
#   * cmx_erf: 4.2e-7 absolute (csrc/cmx_common.h, test_oracle_kats.py::test_fast_erf_table), with the
#     hardware's 1-ulp reciprocal in place of a correctly rounded division: + 2^-23 (|erf| <= 1);
#   * its argument v / sqrt(2) carries two fp32 roundings (the constant, the product): relative
#     2^-23, and |d erf / dt| * |t| = 2 / sqrt(pi) * |t| exp(-t^2) <= 0.484, so + 0.484 * 2^-23 = 5.8e-8;
#   * 1 + erf (<= 2) rounds once, the product with 0.5 v (exact) once: 2 * 2 * 2^-24 = 2^-22 on the bracket;
# all multiplied by 0.5 |v|.  (A fused multiply-add only removes roundings.)  A 16-bit store then
# rounds the fp32 y, |y| <= |ref| + delta: u * (|ref| + delta) with u = 2^-8 (bf16) / 2^-11 (fp16);
# the (1 + 2^-8) factor below carries the u * delta part, so the bound is delta(v) + u * |ref|
# (fp16: at least half the subnormal spacing, 2^-25, for results below 2^-14).
GELU_ERF_ABS = 4.2e-7 + 2.0 ** -23 + 5.8e-8
GELU_REL = 0.5 * (GELU_ERF_ABS + 2.0 ** -22) * (1 + 2.0 ** -8)
STORE_U = {"float32": 0.0, "bfloat16": 2.0 ** -8, "float16": 2.0 ** -11}
STORE_ABS = {"float32": 0.0, "bfloat16": 0.0, "float16": 2.0 ** -25}


def gelu_delta(v):
    """bound on |fp32 kernel GELU(v) - fp64 erf-GELU(v)| for an exact pre-activation v (tensor or array)"""
    return GELU_REL * abs(v)


def gelu_vmax():
    """largest |pre-activation| any GELU case can produce: 4 K + 4"""
    ks = [r.case.K for r in runs() if r.epi == "gelu"]
    return 4 * max(ks) + 4


# --------------------------------------------------------------------- the operand contract
def fast_ok(A, A2, B, M, N, K, tA, tB, ones_col=0):
    """gemm_kernels.h's fast_ok on the tensors a test passes (16-bit operands): whether the launch
    takes the LDS-DMA path a case's variant was planned for"""
    from rgbx_semantic_segmentation_amd.kernels import _operand
    _, lda, sA = _operand(A, "A")
    _, ldb, sB = _operand(B, "B")
    nb = N - 1 if ones_col else N
    if any(t.data_ptr() % 16 for t in (A, B) + ((A2,) if A2 is not None else ())):
        return False
    if lda % 8 or ldb % 8 or sA % 8 or sB % 8 or (K % 8 and not (tA and tB)):
        return False
    if (tA and M % 8) or (tB and nb % 8):
        return False
    if A2 is not None and (A.shape[2] % 64 or A2.stride(1) % 8 or A2.stride(0) % 8 or tA):
        return False
    return True


# ------------------------------------------------------------------------- inputs and buffers
_cache = {}


def exact_product(G, M, N, K, dev):
    """A (G, M, K), B (G, N, K) of {-2, -1, 1, 2} and A B^T, all fp64 on `dev`; the last shape is
    kept, so the epilogues and dtypes of one case share one reference and leave it unchanged"""
    import torch
    key = (G, M, N, K, str(dev))
    if key not in _cache:
        _cache.clear()
        gen = torch.Generator(device=dev).manual_seed(1000003 * M + 1009 * N + K + G)
        vals = torch.tensor([-2.0, -1.0, 1.0, 2.0], dtype=torch.float64, device=dev)
        A = vals[torch.randint(0, 4, (G, M, K), device=dev, generator=gen)]
        B = vals[torch.randint(0, 4, (G, N, K), device=dev, generator=gen)]
        acc = torch.bmm(A, B.transpose(1, 2))
        assert_fp32_exact(acc, "A B^T")
        _cache[key] = (A, B, acc)
    return _cache[key]


def assert_fp32_exact(ref64, what):
    """the premise of an exact comparison, checked on the reference alone"""
    assert bool((ref64.float().double() == ref64).all()), f"test setup: {what} is not exactly representable in fp32"


def operand(X, trans, dtype):
    """logical (G, rows, K) fp64 X as a guarded operand view: the buffer's padding columns
    (ld = K + 8; transposed: ld = rows + 8) and GUARD_ROWS rows past the last are NaN"""
    import torch
    G, R, K = X.shape
    if trans:
        buf = torch.full((G, K + GUARD_ROWS, R + 8), float("nan"), dtype=dtype, device=X.device)
        buf[:, :K, :R] = X.transpose(1, 2).to(dtype)
        return buf[:, :K, :R].transpose(1, 2)
    buf = torch.full((G, R + GUARD_ROWS, K + 8), float("nan"), dtype=dtype, device=X.device)
    buf[:, :R, :K] = X.to(dtype)
    return buf[:, :R, :K]


def guarded(G, M, N, cvec, dtype, dev, fill=None, contiguous=False):
    """(wide, view): `view` (G, M, N) = columns [8, 8 + N) of rows [0, M) of a (G, M + GUARD_ROWS,
    ldc) buffer of SENTINEL, ldc keeping rows 16-B aligned in every dtype (`cvec`) or odd (the
    scalar epilogue; the base stays 16-B aligned, which the mask needs); `contiguous` (G = 1): rows of
    exactly N columns, guard rows only.  `fill` (fp64, exact in `dtype`) initialises the view."""
    import torch
    ldc = N if contiguous else (N + 7) // 8 * 8 + 16 + (0 if cvec else 1)
    wide = torch.full((G, M + GUARD_ROWS, ldc), SENTINEL, dtype=dtype, device=dev)
    view = wide[:, :M, :] if contiguous else wide[:, :M, 8:8 + N]
    if fill is not None:
        view.copy_(fill.to(dtype))
    return wide, view


def check_guarded(wide, view, want, what):
    """`view` holds `want` bit for bit and every other element of `wide` is still the sentinel"""
    import torch
    inside = torch.zeros_like(wide, dtype=torch.bool)
    inside.as_strided(view.shape, view.stride(), view.storage_offset() - wide.storage_offset()).fill_(True)
    assert bool((wide[~inside] == SENTINEL).all()), f"{what}: a guard element around the (M, N) slice was overwritten"
    if want is not None:
        bad = (view != want) | view.isnan()
        assert not bool(bad.any()), (
            f"{what}: {int(bad.sum())} elements differ, first (g, row, col) = {bad.nonzero()[0].tolist()}: got "
            f"{view[bad][0].item()}, want {want[bad][0].item()}")
        assert torch.equal(view, want), what


class Problem:
    """one GEMM of the table on the device: guarded operands, the epilogue's tensors, the
    K.gemm keyword arguments and the fp64 reference"""

    def __init__(self, G, M, N, K, tA, tB, epi, dtype, dev, cvec=True, contiguous=False):
        import torch
        e = EPIS[epi]
        self.G, self.M, self.N, self.K, self.epi, self.e, self.dtype = G, M, N, K, epi, e, dtype
        A, B, acc = exact_product(G, M, N, K, dev)
        gen = torch.Generator(device=dev).manual_seed(77 + len(epi) + M)

        def ints(lo, hi, *shape):
            return torch.randint(lo, hi + 1, shape, device=dev, generator=gen).double()

        self.out_mode = e.get("out_mode", 0)
        cdt = dtype if self.out_mode == 0 else torch.float32
        self.cdt = cdt
        kw = dict(out_mode=self.out_mode, act=e.get("act", "none"))
        if e.get("a2"):
            assert not tA
            K1 = max(64, K // 128 * 64)                # a k-tile boundary near the middle
            kw["A"], kw["A2"] = operand(A[:, :, :K1], 0, dtype), operand(A[:, :, K1:], 0, dtype)
        else:
            kw["A"] = operand(A, tA, dtype)
        kw["B"] = operand(B, tB, dtype)
        v = acc
        if e.get("bias"):
            bias = ints(-16, 16, G, N) / 4
            bbuf = torch.full((G, N + 5), SENTINEL, dtype=torch.float32, device=dev)
            bbuf[:, :N] = bias.float()
            kw["bias"] = bbuf[:, :N] if e["bias"] == "strided" else bbuf[:, :N].contiguous()
            v = v + bias[:, None, :]
        self.pre = v                                   # the exact pre-activation
        assert_fp32_exact(v, "the pre-activation")
        act = kw["act"]
        if act == "relu":
            v = v.clamp_min(0)
        elif act == "gelu":
            v = 0.5 * v * (1 + torch.erf(v * 0.5 ** 0.5))
        c0 = ints(-8, 8, G, M, N) if (e.get("res") == "inplace" or self.out_mode == 2) else None
        self.wide, self.C = guarded(G, M, N, cvec, cdt, dev, c0, contiguous)
        kw["C"] = self.C
        self.Rwide = self.Mwide = None
        if e.get("res"):
            if e["res"] == "inplace":
                r, kw["residual"] = c0, self.C
            else:
                r = ints(-8, 8, G, M, N)
                self.Rwide, kw["residual"] = guarded(G, M, N, cvec, cdt, dev, r, contiguous)
                self.Rwide0 = self.Rwide.clone()
            s = torch.ones(G * M, dtype=torch.float64, device=dev)
            if e.get("rscale"):
                table = torch.tensor([0.0, 0.5, 1.0, 1.25], dtype=torch.float64, device=dev)
                sc = table[torch.randint(0, 4, ((G * M + RPS - 1) // RPS,), device=dev, generator=gen)]
                kw["rscale"], kw["rows_per_sample"] = sc.float(), RPS
                s = sc.repeat_interleave(RPS)[:G * M]
            v = r + s.view(G, M, 1) * v
        if e.get("mask"):
            m = ints(-1, 2, G, M, N)
            self.Mwide, kw["mask"] = guarded(G, M, N, cvec, cdt, dev, m, contiguous)
            self.Mwide0 = self.Mwide.clone()
            v = torch.where(m > 0, v, torch.zeros_like(v))
        if self.out_mode == 2:
            v = c0 + v
        self.dbwide = None
        if e.get("dbias"):
            d0 = ints(-8, 8, G, M)
            self.dbwide = torch.full((G, M + 8), SENTINEL, dtype=torch.float32, device=dev)
            self.dbwide[:, :M] = d0.float()
            kw["dbias"] = self.dbwide[:, :M]
            self.dbref = A.sum(2) + (d0 if self.out_mode == 2 else 0)
            assert_fp32_exact(self.dbref, "the bias gradient")
        self.ref = v
        self.exact = act != "gelu"
        if self.exact:
            assert_fp32_exact(v, "the epilogue's result")
        self.kw = kw

    def check(self, what):
        """after the launch: C against the reference (exactly, or inside the GELU bound), every
        guard and every read-only tensor untouched"""
        import torch
        M, N = self.M, self.N
        name = str(self.cdt).replace("torch.", "")
        if self.exact:
            check_guarded(self.wide, self.C, self.ref.float().to(self.cdt), what)
        else:
            check_guarded(self.wide, self.C, None, what)
            err = (self.C.double() - self.ref).abs()
            bound = gelu_delta(self.pre) + torch.clamp(STORE_U[name] * self.ref.abs(), min=STORE_ABS[name])
            worst = (err - bound).max().item()
            print(f"{what}: max |y - ref| = {err.max().item():.3e}, max (err - bound) = {worst:.3e}, "
                  f"max err / bound = {(err / bound.clamp_min(1e-300)).max().item():.3f}")
            assert not bool(self.C.isnan().any()) and worst <= 0, what
        if self.Rwide is not None:
            assert torch.equal(self.Rwide, self.Rwide0), f"{what}: the residual was written"
        if self.Mwide is not None:
            assert torch.equal(self.Mwide, self.Mwide0), f"{what}: the mask was written"
        if self.dbwide is not None:
            assert torch.equal(self.dbwide[:, :M], self.dbref.float()), f"{what}: bias gradient"
            assert bool((self.dbwide[:, M:] == SENTINEL).all()), f"{what}: bias-gradient guard overwritten"
