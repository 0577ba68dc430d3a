"""Inputs and references of the SRA attention tests: one table of cases, read by
tests/test_sra_cases.py (CPU: the constructions' preconditions hold on the references alone) and by
tests/test_gpu_sra.py (GPU: every kernel variant, asserted through kernels.sra_plan).

Every reference is fp64 torch on the rounded inputs (softmax(q k^T D^-1/2) v of
dual_segformer.py:125-134 and its autograd backward), and also returns lse, the natural-log
logsumexp of the scaled scores (what the kernels store: (m + log2 l) ln 2).

Input kinds.
  random / peaked  Gaussian q (x 6 for peaked: the online-softmax rescale decides the result), kv, dO.
  selector         a one-hot softmax whose results are exact.  Key j = e[j % h] + e[h + j // h] with
                   h = D / 2 (D = 64: Nk <= 1024; D = 32: Nk <= 256), query i = 1024 x key t(i),
                   scale = D^-1/2.  At D = 64 the scaled scores are 256 (the target), 128 (one shared
                   index) or 0, so the off-target probabilities are at most e^-128: zero in fp32
                   (exp2 of -184 underflows) and below 2^-30 in fp64.  V holds integers of [-8, 8],
                   dO of [-4, 4]: o = v[t(i)], lse = 256 (2048 scale in general), dq = dk = 0 (dS =
                   P (dP - D) with dP = D exactly on the target and P = 0 elsewhere), and dv[j] = the
                   sum of the dO rows that target j, an integer that fp32 accumulates exactly in any
                   order; the one rounding is the 16-bit store.  Targets are random, include key 0
                   and key Nk - 1 (N > 1), and the last query row targets key Nk - 1: a key dropped or a
                   padded key admitted at either end of a ragged tile changes an exact result.
  uniform          q = 0: every probability is 1 / Nk, o is the column mean of V (integers) and
                   lse = ln Nk.  One phantom key (a padded row that escapes the tail mask) moves lse
                   by ln((Nk + 1) / Nk) ~ 1 / Nk >= 9.8e-4 at Nk <= 1024, 50 x the 2e-5 bound.  k
                   holds multiples of 1/8 in [-4, 4]: exact in bf16 and fp16.

Emulated yardstick (emulate): the fp32 restatement of a 16-bit flash backward -- P and dS rounded to
the storage type before their matrix products (every MFMA operand is 16-bit), o and the gradients
rounded on store.  Its error against fp64, per tensor and relative to max |ref|, is E_emul; a
correct kernel differs from it in summation order only, so the GPU bound is 2 E_emul + one ulp (the
margin tests/test_gpu_kernels.py::test_sra_fwd_kernel_choice gives two correct summation orders)."""
from __future__ import annotations

import contextlib
import functools
import math
from collections import namedtuple
from dataclasses import dataclass, field

import torch

KNOB_DEFAULTS = dict(SRA_SMALL_FWD_N=600, SRA_SMALL_N=2048, SRA_DQ_SEQ=1, SRA_QW=0, SRA_NW=0, SRA_DKV_DIRECT=0)
NUM_CU = 256                                   # the CU count the B2 plans are pinned at (MI355X)
# one output ulp relative to the output scale (fp32: the suite's fp32 tolerance)
ULP = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 1e-4}
H16 = (torch.bfloat16, torch.float16)
KINDS = ("random", "peaked", "selector", "uniform")
PAD_ROWS = 320                                 # containment: rows of padding around every tensor
SENTINEL = -3072.0                             # exact in bf16 / fp16 / fp32


@dataclass(frozen=True, eq=False)          # cases are module-level singletons: identity hash
class Case:
    name: str
    Bt: int
    N: int
    Nk: int
    heads: int
    D: int = 64
    knobs: dict = field(default_factory=dict)     # overrides of KNOB_DEFAULTS (without the SRA_ prefix)
    plan: dict = field(default_factory=dict)      # the fields of kernels.sra_plan the case is meant for
    dtypes: tuple = H16
    kinds: tuple = KINDS
    both_dq: bool = False                          # small backward: run SRA_DQ_SEQ 0 and 1

    @property
    def C(self):
        return self.heads * self.D


FORCE_LDS = dict(SMALL_FWD_N=0, SMALL_N=0)         # keep short sequences off the small kernels
QWNW = ((2, 4), (2, 8), (1, 10), (1, 8), (1, 4), (1, 2))


def _fast_cases():
    out = []
    for qw, nw in QWNW:
        for Nk in (300, 650):                      # one LDS chunk / three streamed ones, both ragged
            N = 64 * qw * nw + 37                  # two full workgroups and a ragged tail
            out.append(Case(f"fast_qw{qw}_nw{nw}_Nk{Nk}", 2, N, Nk, 2, knobs=dict(FORCE_LDS, QW=qw, NW=nw),
                            plan=dict(fwd="fast", bwd="fast", qw=qw, nw=nw, dkv_direct=False)))
    for Nk in (300, 650):
        out.append(Case(f"fast_dkv_direct_Nk{Nk}", 2, 197, Nk, 2, knobs=dict(FORCE_LDS, DKV_DIRECT=197),
                        plan=dict(fwd="fast", bwd="fast", dkv_chunks=1, dkv_direct=True)))
    out.append(Case("fast_dkv_4chunks", 2, 197, 300, 2, knobs=FORCE_LDS,
                    plan=dict(bwd="fast", dkv_chunks=4, dkv_direct=False)))
    out.append(Case("fast_dkv_10chunks", 2, 577, 300, 2, knobs=FORCE_LDS,          # ragged over the reducer's 4 slices
                    plan=dict(bwd="fast", dkv_chunks=10, dkv_direct=False)))
    out.append(Case("fast_dkv_64cap", 1, 4097, 70, 1,                              # 65 query tiles, 64 chunks
                    plan=dict(fwd="fast", bwd="fast", dkv_chunks=64, dkv_direct=False)))
    return out


# (N, Nk): 1, 3, 9 and 10 query tiles through the 8-wave dK / dV; one- to five-wave key splits
SMALL_SHAPES = ((1, 1), (1, 320), (37, 33), (64, 64), (65, 65), (129, 257), (129, 33), (37, 257), (65, 320),
                (577, 1), (577, 65), (577, 320))


def _small_cases():
    # Nk = 1: the softmax is the constant 1, so dq = dk = 0 by cancellation (dP - D) and Gaussian data
    # leaves only fp32 noise against a zero reference; the selector and the uniform kind, whose
    # cancellation is exact, hold that shape
    return [Case(f"small_N{N}_Nk{Nk}", 2, N, Nk, 2, both_dq=True, kinds=KINDS if Nk > 1 else ("selector", "uniform"),
                 plan=dict(fwd="small", bwd="small", dkv_direct=True)) for N, Nk in SMALL_SHAPES]


def _general_cases():
    gen = dict(fwd="general", bwd="general", dkv_direct=False)
    f32 = (torch.float32,)
    sel = ("random", "peaked", "uniform")          # the selector is specified for fp32 on this path
    return [Case("general_333x70_D32_f32", 2, 333, 70, 2, D=32, plan=gen, dtypes=f32),
            Case("general_65x80_D32_f32", 1, 65, 80, 8, D=32, plan=gen, dtypes=f32),
            Case("general_333x70_D64_f32", 2, 333, 70, 2, D=64, plan=gen, dtypes=f32),
            Case("general_333x70_D32_h16", 2, 333, 70, 2, D=32, plan=gen, kinds=sel),
            Case("general_65x80_D32_h16", 1, 65, 80, 8, D=32, plan=gen, kinds=sel)]


MATRIX = _fast_cases() + _small_cases() + _general_cases()

# default knobs on both sides of every threshold
THRESHOLDS = [
    Case("thr_Nk320", 1, 129, 320, 2, plan=dict(fwd="small", bwd="small"), kinds=("random",)),
    Case("thr_Nk321", 1, 129, 321, 2, plan=dict(fwd="fast", bwd="fast"), kinds=("random",)),
    Case("thr_N600", 1, 600, 300, 2, plan=dict(fwd="small", bwd="small"), kinds=("random",)),
    Case("thr_N601", 1, 601, 300, 2, plan=dict(fwd="fast", bwd="small"), kinds=("random",)),
    Case("thr_N2048", 1, 2048, 300, 2, plan=dict(fwd="fast", bwd="small"), kinds=("random",)),
    Case("thr_N2049", 1, 2049, 300, 2, plan=dict(fwd="fast", bwd="fast"), kinds=("random",)),
]

# one ragged shape per kernel: fast forward / dQ at (1, 2) with the slab dK / dV and its reducer, at
# (2, 4) with the direct dK / dV; the three small kernels with both dQ forms; the general kernels
CONTAINMENT = [
    Case("contain_fast_slab", 2, 165, 300, 2, knobs=dict(FORCE_LDS, QW=1, NW=2),
         plan=dict(fwd="fast", bwd="fast", qw=1, nw=2, dkv_chunks=3, dkv_direct=False)),
    Case("contain_fast_direct", 2, 549, 650, 2, knobs=dict(FORCE_LDS, QW=2, NW=4, DKV_DIRECT=549),
         plan=dict(fwd="fast", bwd="fast", qw=2, nw=4, dkv_chunks=1, dkv_direct=True)),
    Case("contain_small", 2, 129, 257, 2, both_dq=True, plan=dict(fwd="small", bwd="small")),
    Case("contain_general", 2, 333, 70, 2, D=32, plan=dict(fwd="general", bwd="general"),
         dtypes=(torch.float32, torch.bfloat16, torch.float16)),
]

# the four SRA shapes of B2 at 480 x 640, bs = 2 (Bt = 2 modalities x 2), at 256 CUs
B2_PINS = [
    ("stage1", (4, 19200, 300, 1), dict(fwd="fast", qw=1, nw=10, bwd="fast", dkv_chunks=64, dkv_direct=False)),
    ("stage2", (4, 4800, 300, 2), dict(fwd="fast", qw=1, nw=8, bwd="fast", dkv_chunks=32, dkv_direct=False)),
    ("stage3", (4, 1200, 300, 5), dict(fwd="fast", qw=1, nw=2, bwd="small")),
    ("stage4", (4, 300, 300, 8), dict(fwd="small", bwd="small")),
]


# ------------------------------------------------------------------------- knobs and the plan
@contextlib.contextmanager
def knobs(**over):
    """every SRA knob at its default, `over` (names without SRA_) on top, for the launches inside;
    the values found before (or the defaults, for knobs nothing had read yet) are put back"""
    from rgbx_semantic_segmentation_amd import kernels as K
    want = dict(KNOB_DEFAULTS)
    for k, v in over.items():
        assert "SRA_" + k in want, k
        want["SRA_" + k] = v
    prev = {k: K.tune_get(k) for k in want}
    try:
        for k, v in want.items():
            K.tune(k, v)
        yield
    finally:
        for k, d in KNOB_DEFAULTS.items():
            K.tune(k, prev[k] if prev[k] >= 0 else d)


def assert_plan(K, case, dtype, **extra):
    """the launch code plans the variant the case names (kernels.sra_plan; nothing is launched)"""
    plan = K.sra_plan(case.Bt, case.N, case.Nk, case.heads, case.D, dtype)
    want = dict(case.plan, **extra)
    got = {k: getattr(plan, k) for k in want}
    assert got == want, f"{case.name}: the launch code plans {plan}, the case is meant for {want}"
    return plan


def runs(cases):
    return [(c, dt, kind) for c in cases for dt in c.dtypes for kind in c.kinds]


def run_id(r):
    c, dt, kind = r
    return f"{c.name}-{str(dt).replace('torch.', '')}-{kind}"


# ------------------------------------------------------------------------------------ inputs
Inputs = namedtuple("Inputs", "q kv do target")    # fp64 tensors holding values exact in the dtype


def _seed(case, kind):
    return sum(ord(ch) for ch in case.name + kind) * 7919 + case.N * 31 + case.Nk


def selector_keys(Nk, D):
    h = D // 2
    assert Nk <= h * h, (Nk, D)
    j = torch.arange(Nk)
    k = torch.zeros(Nk, D, dtype=torch.float64)
    k[j, j % h] = 1.0
    k[j, h + j // h] = 1.0
    return k


def make_inputs(case, kind, dtype):
    """q (Bt, N, C), kv (Bt, Nk, 2C), dO (Bt, N, C) as fp64 tensors whose values are exact in `dtype`;
    target (Bt, heads, N) for the selector."""
    g = torch.Generator().manual_seed(_seed(case, kind))
    Bt, N, Nk, heads, D, C = case.Bt, case.N, case.Nk, case.heads, case.D, case.C
    if kind in ("random", "peaked"):
        rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
        q = rnd(Bt, N, C) * (6.0 if kind == "peaked" else 1.0)
        x = Inputs(q, rnd(Bt, Nk, 2 * C), rnd(Bt, N, C), None)
        return Inputs(*(t.to(dtype).double() for t in x[:3]), None)
    ints = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).double()
    v, do = ints(-8, 8, Bt, Nk, C), ints(-4, 4, Bt, N, C)
    if kind == "uniform":
        k = (torch.randn(Bt, Nk, C, generator=g, dtype=torch.float64) * 8).round().clamp(-32, 32) / 8
        return Inputs(torch.zeros(Bt, N, C, dtype=torch.float64), torch.cat([k, v], -1), do, None)
    assert kind == "selector"
    keys = selector_keys(Nk, D)                                     # (Nk, D), the same for every (b, head)
    t = torch.randint(0, Nk, (Bt, heads, N), generator=g)
    t[..., 0] = 0
    if N > 1:
        t[..., N // 2] = Nk - 1
    t[..., N - 1] = Nk - 1                                          # the last query row: the last key
    q = (1024.0 * keys[t]).permute(0, 2, 1, 3).reshape(Bt, N, C)    # (Bt, heads, N, D) -> token-major
    k = keys[None, :, None, :].expand(Bt, Nk, heads, D).reshape(Bt, Nk, C)
    return Inputs(q, torch.cat([k, v], -1), do, t)


# -------------------------------------------------------------------------------- references
Result = namedtuple("Result", "o lse dq dkv")      # o, dq (Bt, N, C); lse (Bt, heads, N); dkv (Bt, Nk, 2C)


def _heads(x, heads, D):
    Bt, R, _ = x.shape
    return x.view(Bt, R, heads, D).transpose(1, 2)                   # (Bt, heads, R, D)


def _tokens(x):
    Bt, heads, R, D = x.shape
    return x.transpose(1, 2).reshape(Bt, R, heads * D)


def reference(x, heads, D):
    """fp64 autograd on the given (already rounded) inputs."""
    C = heads * D
    q = x.q.clone().requires_grad_(True)
    kv = x.kv.clone().requires_grad_(True)
    s = (_heads(q, heads, D) @ _heads(kv[..., :C], heads, D).transpose(-2, -1)) * D ** -0.5
    o = _tokens(s.softmax(-1) @ _heads(kv[..., C:], heads, D))
    o.backward(x.do)
    return Result(o.detach(), torch.logsumexp(s.detach(), -1), q.grad, kv.grad)


def emulate(x, heads, D, dtype):
    """fp32 restatement of a flash forward / backward that stores `dtype`: the unnormalised P of the
    forward, and P and dS of the backward, are rounded to `dtype` before their matrix products; o,
    dq, dk, dv are rounded on store (the backward reads the rounded o)."""
    C = heads * D
    rnd = lambda t: t.to(dtype).float()
    scale = torch.tensor(D ** -0.5, dtype=torch.float32)
    q, k, v = (_heads(t.float(), heads, D) for t in (x.q, x.kv[..., :C], x.kv[..., C:]))
    do = _heads(x.do.float(), heads, D)
    s = (q @ k.transpose(-2, -1)) * scale
    m = s.max(-1, keepdim=True).values
    pu = (s - m).exp()
    l = pu.sum(-1, keepdim=True)
    o = rnd((rnd(pu) @ v) / l)
    lse = (m + l.log()).squeeze(-1)
    p = (s - lse.unsqueeze(-1)).exp()
    dsum = (do * o).sum(-1, keepdim=True)
    ds = rnd(p * (do @ v.transpose(-2, -1) - dsum))
    dq = rnd((ds @ k) * scale)
    dk = rnd((ds.transpose(-2, -1) @ q) * scale)
    dv = rnd(rnd(p).transpose(-2, -1) @ do)
    return Result(_tokens(o), lse, _tokens(dq), torch.cat([_tokens(dk), _tokens(dv)], -1))


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


def grads(r, C):
    return dict(dq=r.dq, dk=r.dkv[..., :C], dv=r.dkv[..., C:])


def selector_expected(case, x, dtype):
    """o = v[t], lse = 2048 D^-1/2, dq = dk = 0, dv = the scatter-sum of dO (fp64, rounded once)."""
    Bt, N, Nk, heads, D, C = case.Bt, case.N, case.Nk, case.heads, case.D, case.C
    v, do, t = _heads(x.kv[..., C:], heads, D), _heads(x.do, heads, D), x.target
    o = torch.gather(v, 2, t[..., None].expand(Bt, heads, N, D))
    dv = torch.zeros(Bt, heads, Nk, D, dtype=torch.float64).scatter_add_(2, t[..., None].expand(Bt, heads, N, D), do)
    return Result(_tokens(o), torch.full((Bt, heads, N), 2048.0 * D ** -0.5, dtype=torch.float64),
                  torch.zeros(Bt, N, C, dtype=torch.float64),
                  torch.cat([torch.zeros(Bt, Nk, C, dtype=torch.float64), _tokens(dv).to(dtype).double()], -1))


Expected = namedtuple("Expected", "x ref e_emul")


@functools.lru_cache(maxsize=None)
def expected(case, kind, dtype):
    """Inputs, fp64 reference and E_emul (per gradient tensor) of one run: computed once, shared by
    the tests that need it, never modified."""
    x = make_inputs(case, kind, dtype)
    ref = reference(x, case.heads, case.D)
    emu = emulate(x, case.heads, case.D, dtype)
    ge, gr = grads(emu, case.C), grads(ref, case.C)
    return Expected(x, ref, {n: relerr(ge[n], gr[n]) for n in gr})


def bwd_bound(e_emul, dtype):
    return 2 * e_emul + ULP[dtype]


def uniform_lse(Nk):
    return math.log(Nk)
