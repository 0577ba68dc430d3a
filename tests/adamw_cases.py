"""Inputs, references and bounds of the AdamW kernel tests (csrc/adamw.hip).  No GPU, no HIP:
tests/test_adamw_cases.py checks these constructions on the CPU, tests/test_gpu_adamw.py runs the
kernels against them through the C-ABI.

Reference: ``torch.optim.AdamW(..., foreach=False)`` on the CPU in fp64 over the flag-1 (decay) and
flag-0 (no decay) elements as two groups; the frozen (flag-2) elements are in no group.

Bound of a tensor (p, m, v) at a step: ``2 E_ref + u max|ref|``.  E_ref is the worst absolute error
of the same torch run in fp32 against the fp64 run over the non-frozen elements and u = 2^-23: the
project's "2 E + one ulp" with torch's own fp32 optimizer as the yardstick.  Bit equality with torch
is not asked (either side may or may not fuse its multiply-adds).

Moved condition: at every step of every case the median |dp| of the fp64 reference over the
non-frozen elements is at least MOVED x the bound of p, so a skipped or no-op step cannot pass.
"""
import functools
import math

import numpy as np
import torch

U = 2.0 ** -23
MOVED = 100
GUARD = 64
# NaN bit patterns of the guards (a stray write, or a read that reaches the arithmetic, shows)
NAN32 = 0x7FC0DEAD
NAN16 = {torch.bfloat16: 0x7FC1, torch.float16: 0x7E01}
SHADOW_INIT = 0x1234            # what the shadow holds before the first step (live: overwritten; frozen: stays)
MV_FROZEN = 7.0                 # what the frozen blocks of m and v hold (must stay)
T_RESUME = 9999
LOSS_SCALE = 3000.0             # not a power of two

# name: (n, grid cap).  Blocks are 256 threads of one float4: 64000 -> 63 blocks, 131136 -> 129 blocks
SIZES = {
    "n64": (64, 0),                      # one block, tail path only
    "n1088": (1088, 0),                  # two blocks, tail only
    "n64000_cap3": (64000, 3),           # unrolled loop plus a partial tail
    "n64000": (64000, 0),                # 63 blocks, one partial ticket group
    "n131136": (131136, 0),              # 129 blocks: groups of 64, 64 and 1
    "n131136_cap65": (131136, 65),       # groups of 64 and 1; some threads only loop, others only take the tail
}
SHADOWS = {"noshadow": None, "bf16": torch.bfloat16, "fp16": torch.float16}
SHADOW_CODE = {None: 0, torch.bfloat16: 1, torch.float16: 2}

_LRS = (1e-3, 5e-4, 2e-3, 1e-3)          # changes every step: lr is a device scalar
HYPER = {
    "default": dict(betas=(0.9, 0.999), eps=1e-8, wd=0.01, lrs=_LRS),
    "alt": dict(betas=(0.8, 0.95), eps=1e-6, wd=0.1, lrs=_LRS),
    "project_lr": dict(betas=(0.9, 0.999), eps=1e-8, wd=0.01, lrs=(6e-5, 6e-5, 3e-5, 6e-5)),
}
STARTS = ("fresh", "resume")

# (size, hyper, start, loss scale) of every reference the GPU test uses
CASES = [(s, "default", "fresh", None) for s in SIZES]
CASES += [(s, h, "fresh", None) for h in ("alt", "project_lr") for s in ("n1088", "n131136")]
CASES += [(s, h, "resume", None) for h in ("default", "project_lr") for s in ("n1088", "n64000")]
CASES += [(s, "default", "fresh", LOSS_SCALE) for s in ("n1088", "n64000")]


def case_id(c):
    size, hyper, start, scale = c
    return f"{size}-{hyper}-{start}" + (f"-S{scale:g}" if scale else "")


def flags(n):
    """the per-64-element flag: 1 = decay, 0 = no decay, 2 = frozen"""
    return torch.tensor([(1, 0, 2)[b % 3] for b in range(n // 64)], dtype=torch.uint8)


@functools.lru_cache(maxsize=None)
def inputs(n):
    """p ~ 0.05 N(0,1); four g ~ 0.02 N(0,1) with g[5] = 0, g[7] = 1e-30 (g^2 underflows in fp32) and
    NaN in the frozen blocks; the per-element flags; the resume state m0 ~ 0.01 N, v0 = (0.02 N)^2."""
    gen = torch.Generator().manual_seed(1234 + n)
    p = 0.05 * torch.randn(n, generator=gen)
    gs = [0.02 * torch.randn(n, generator=gen) for _ in _LRS]
    m0 = 0.01 * torch.randn(n, generator=gen)
    v0 = (0.02 * torch.randn(n, generator=gen)) ** 2
    fe = flags(n).repeat_interleave(64)
    for g in gs:
        g[5], g[7] = 0.0, 1e-30
        g[fe == 2] = float("nan")
    return p, gs, fe, m0, v0


def start_state(n, start):
    """(m, v, step count) the kernel starts from: the frozen blocks of m and v hold MV_FROZEN"""
    _, _, fe, m0, v0 = inputs(n)
    frozen = fe == 2
    if start == "fresh":
        m, v, t = torch.zeros(n), torch.zeros(n), 0
    else:
        m, v, t = m0.clone(), v0.clone(), T_RESUME
    m[frozen] = MV_FROZEN
    v[frozen] = MV_FROZEN
    return m, v, t


def torch_adamw(p, gs, fe, hyper, dtype, m0=None, v0=None, t0=0, gmul=None):
    """torch.optim.AdamW over the flag-1 and flag-0 elements as two groups (the frozen ones are in no
    group); [(p, m, v, step)] after every step, scattered back to flat order.  A start state is
    loaded through load_state_dict, the way a checkpoint would be.  gmul: g is multiplied by it in
    `dtype` first (GradScaler.unscale_)."""
    h = HYPER[hyper]
    sel = [fe == 1, fe == 0]
    params = [torch.nn.Parameter(p[k].to(dtype).clone()) for k in sel]
    groups = [dict(params=[params[0]]), dict(params=[params[1]], weight_decay=0.0)]
    opt = torch.optim.AdamW(groups, lr=h["lrs"][0], betas=h["betas"], eps=h["eps"], weight_decay=h["wd"], foreach=False)
    if t0:
        sd = opt.state_dict()
        sd["state"] = {i: dict(step=torch.tensor(float(t0)), exp_avg=m0[k].clone(), exp_avg_sq=v0[k].clone())
                       for i, k in enumerate(sel)}
        opt.load_state_dict(sd)
    out = []
    for lr, g in zip(h["lrs"], gs):
        for grp in opt.param_groups:
            grp["lr"] = lr
        for q, k in zip(params, sel):
            q.grad = g[k].to(dtype) if gmul is None else g[k].to(dtype) * gmul
        opt.step()
        pf = p.to(dtype).clone()
        mf, vf = torch.zeros(p.numel(), dtype=dtype), torch.zeros(p.numel(), dtype=dtype)
        for q, k in zip(params, sel):
            pf[k] = q.detach()
            mf[k] = opt.state[q]["exp_avg"]
            vf[k] = opt.state[q]["exp_avg_sq"]
        steps = {float(opt.state[q]["step"]) for q in params}
        assert len(steps) == 1
        out.append((pf, mf, vf, steps.pop()))
    return out


def kernel_grads(n, scale=None):
    """the gradients handed to the kernel: g, or fp32(g S) with a loss scale S"""
    gs = inputs(n)[1]
    return gs if scale is None else [g * scale for g in gs]


@functools.lru_cache(maxsize=None)
def reference(n, hyper, start="fresh", scale=None):
    """Per step: dict(p, m, v fp64; bound_p, bound_m, bound_v; moved = median |dp| over the non-frozen
    elements; step).  With a loss scale S the fp64 run steps on gs.double() / S, the exact value of
    what the kernel was given, and the fp32 run on gs * fp32(1 / S), as GradScaler.unscale_ does."""
    p, _, fe, m0, v0 = inputs(n)
    gk = kernel_grads(n, scale)
    t0 = T_RESUME if start == "resume" else 0
    kw = dict(m0=m0, v0=v0, t0=t0)
    if scale is None:
        r64 = torch_adamw(p, gk, fe, hyper, torch.float64, **kw)
        r32 = torch_adamw(p, gk, fe, hyper, torch.float32, **kw)
    else:
        r64 = torch_adamw(p, [g.double() / scale for g in gk], fe, hyper, torch.float64, **kw)
        r32 = torch_adamw(p, gk, fe, hyper, torch.float32, gmul=torch.tensor(1.0 / scale, dtype=torch.float32), **kw)
    live = fe != 2
    out, prev = [], p.double()
    for (p64, m64, v64, t), (p32, m32, v32, _) in zip(r64, r32):
        d = dict(p=p64, m=m64, v=v64, step=t)
        for name, a64, a32 in (("p", p64, p32), ("m", m64, m32), ("v", v64, v32)):
            e_ref = (a32.double() - a64)[live].abs().max().item()
            d["bound_" + name] = 2 * e_ref + U * a64[live].abs().max().item()
        d["moved"] = (p64 - prev)[live].abs().median().item()
        out.append(d)
        prev = p64
    return out


def restate_kernel(p, gs, fe, hyper, m, v, t0, grad_scale=1.0, loss_scale=None):
    """adamw_kernel's own formula in fp32 NumPy: the step's scalars formed in double from the fp32 lr
    and rounded once, then the per-element update in the kernel's order.  [(p, m, v, step)] per
    step.  For the CPU test only."""
    f32 = np.float32
    h = HYPER[hyper]
    b1d, b2d = h["betas"]
    eps, wd = f32(h["eps"]), h["wd"]
    omb1, b2, omb2 = f32(1.0 - b1d), f32(b2d), f32(1.0 - b2d)
    live = (fe != 2).numpy()
    decays = (fe == 1).numpy()
    p, m, v = (a.numpy().astype(f32).copy() for a in (p, m, v))
    gscale = f32(grad_scale) / f32(loss_scale) if loss_scale is not None else f32(grad_scale)
    t, out = float(t0), []
    with np.errstate(invalid="ignore", under="ignore"):
        for lr, g in zip(h["lrs"], gs):
            lrd = float(f32(lr))                                # the device scalar is an fp32
            t += 1.0
            step_size = f32(lrd / (1.0 - math.pow(b1d, t)))
            bc2s = f32(math.sqrt(1.0 - math.pow(b2d, t)))
            decf = f32(1.0 - lrd * wd)
            gj = g.numpy().astype(f32) * gscale
            pa = p * np.where(decays, decf, f32(1.0))
            ma = m + omb1 * (gj - m)
            va = v * b2 + omb2 * gj * gj
            denom = np.sqrt(va) / bc2s + eps
            pa = pa - step_size * (ma / denom)
            p, m, v = (np.where(live, new, old).astype(f32) for new, old in ((pa, p), (ma, m), (va, v)))
            out.append((torch.from_numpy(p.copy()), torch.from_numpy(m.copy()), torch.from_numpy(v.copy()), t))
    return out


# ------------------------------------------------------------------ the loss scale
SCALE_SEQUENCE = (0, 0, 1, 0, 0, 0, 0, 1, 1, 0, 0, 0)      # found_inf before each update
SCALE_START = dict(scale=2.0 ** 10, growth=2.0, backoff=0.5, interval=3)


def loss_scale_update(scale, tracker, found, growth, backoff, interval):
    """loss_scale_update_kernel in plain Python: (scale, tracker, found) after the call"""
    if found != 0:
        scale, tracker = scale * backoff, 0
    else:
        tracker += 1
        if tracker >= interval:
            scale, tracker = scale * growth, 0
    return scale, tracker, 0.0


def torch_scaler_sequence(seq=SCALE_SEQUENCE, scale=None, growth=None, backoff=None, interval=None):
    """[(scale, growth tracker)] of torch.amp.GradScaler("cpu") after each update of the sequence (a
    one-element SGD whose gradient is inf where the sequence says found_inf)"""
    s = dict(SCALE_START)
    sc = torch.amp.GradScaler("cpu", init_scale=scale or s["scale"], growth_factor=growth or s["growth"],
                              backoff_factor=backoff or s["backoff"], growth_interval=interval or s["interval"])
    w = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([w], lr=0.0)
    out = []
    for found in seq:
        sc.scale(torch.zeros(1))                      # (creates the scale tensor on first use)
        w.grad = torch.full((1,), float("inf") if found else 1.0)
        sc.step(opt)
        sc.update()
        out.append((sc.get_scale(), int(sc._growth_tracker.item())))
    return out


# ------------------------------------------------------------------ cmx_grad_nonfinite
NF_BLOCKS, NF_THREADS = 4096, 256
NF_PASS = NF_BLOCKS * NF_THREADS * 4                       # elements one pass of the capped grid covers
NF_N = NF_PASS + 3 * 64                                    # 4,194,496: a second pass over three 64-blocks
NF_FROZEN = (130, NF_PASS + 64 + 5)                        # inside flag-2 blocks of the first and second pass


def nf_positions(n):
    """where a single non-finite value is placed (all in live blocks): element 0, both sides of a flag
    boundary, 577 (block 9; a flag index off by a factor of four would read block 2's), the last
    element of the first pass, the first of the second, the last element"""
    if n <= NF_PASS:
        return sorted({0, n - 1})
    return [0, 63, 64, 577, NF_PASS - 1, NF_PASS, n - 1]


# ------------------------------------------------------------------ guarded device buffers
class Guarded:
    """A device buffer of n elements with GUARD elements of a NaN bit pattern on both sides."""

    def __init__(self, n, dtype, dev, fill=None):
        self.n, self.dtype = n, dtype
        self.idt, self.pattern = (torch.int32, NAN32) if dtype == torch.float32 else (torch.int16, NAN16[dtype])
        self.raw = torch.full((n + 2 * GUARD,), self.pattern, dtype=self.idt, device=dev)
        self.t = self.raw.view(dtype)[GUARD:GUARD + n]
        if fill is not None:
            self.t.copy_(fill)

    def bits(self):
        return self.raw[GUARD:GUARD + self.n].cpu()

    def guards_intact(self):
        r = self.raw.cpu()
        return bool((r[:GUARD] == self.pattern).all() and (r[GUARD + self.n:] == self.pattern).all())
