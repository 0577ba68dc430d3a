"""Autograd Functions of the CMX training step, each backed by libcmx_hip.so kernels.

Conventions
 * Encoder activations are (G, M, C) tensors, G = 2 modality groups (RGB, X) processed by
   one launch, M = B * H * W tokens (token-major = NHWC), C channels contiguous.
 * Weights arrive as storage-layout views of the ParamStore (stacked over the modality
   pair, compute dtype); their gradients are written directly into the fp32 gradient
   buffer views passed alongside (``Wg``/``bg``).  Functions return ``None`` for those
   and take an ``anchor`` Parameter only so autograd records the node.
 * Every dense GEMM (Linear / 1x1 conv / implicit or im2col conv; fwd, dgrad, wgrad) runs
   on cmx_gemm / cmx_conv_implicit_fwd / the deferred grouped launch (csrc/gemm.hip, MFMA
   bf16 or fp32), with fp32 weight gradients; every other op is a hand-written gfx950
   kernel too (see include/cmx_hip.h).  No library GEMM is on the path.
"""
from __future__ import annotations

import os

import torch
from torch.autograd import Function

from . import deferred
from . import kernels as K


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


def _dgrad(dz, W_slice, out):
    """out (G, M, k) = dz (G, M, N) @ W_slice (G, N, k)."""
    K.gemm(dz, W_slice.transpose(1, 2), out)
    return out


def _wgrad_into(dz, x, Wg_slice, bg=None):
    """Wg_slice (fp32 view (G, N, k)) = dz^T x;  bg (G, N) = column sums of dz.  bf16: queued
    for the segment's grouped weight-gradient launch (deferred.py); otherwise run now."""
    if deferred.wgrad(dz, x, Wg_slice, bg):
        return
    K.gemm(dz.transpose(1, 2), x.transpose(1, 2), Wg_slice, out_mode=1, dbias=bg, splitk=0)


def _fwd_gemm(x, W, b, y, act="none", res=None, rscale=None, rps=1, x2=None):
    K.gemm(x, W, y, bias=b, residual=res, rscale=rscale, rows_per_sample=rps, act=act, A2=x2)
    return y


class GLinear(Function):
    """y[g] = act(x1[g] @ W[g][:, :k1]^T (+ x2[g] @ W[g][:, k1:]^T) + b[g]), optionally
    y = res + rscale[sample] * (...)  (nn.Linear / 1x1 Conv2d; the two-input form replaces
    torch.cat of the inputs, e.g. CrossPath.end_proj on cat(y, v), net_utils.py:277-280,
    ChannelEmbed's 1x1 convs on cat(x1, x2), :323-326; the residual form is Block's
    x + drop_path(proj/fc2(...)), dual_segformer.py:168-169)."""

    @staticmethod
    def forward(ctx, W, Wg, b, bg, anchor, act, res, rscale, rps, x1, x2, tap=None, ln=None, dgrad_tap=None):
        G, N, Ktot = W.shape
        M = x1.shape[1]
        assert x1.shape[-1] + (x2.shape[-1] if x2 is not None else 0) == Ktot, (x1.shape, W.shape)
        y = torch.empty(G, M, N, dtype=x1.dtype, device=x1.device)
        pre = None
        if ln is not None:
            # the consumer LayerNorm of this output in the same launch (cmx_gemm_ln): its result
            # goes to the LNTail, which that norm's LayerNormResF takes instead of launching
            gamma, beta, eps, sink = ln
            pre = K.gemm_ln(x1, W, y, gamma, beta, eps, bias=b, residual=res, rscale=rscale, rows_per_sample=rps,
                            act=act, A2=x2)
            sink.pre = pre
        if pre is None:
            _fwd_gemm(x1, W, b, y, act=act, res=res, rscale=rscale, rps=rps, x2=x2)
        ctx.save_for_backward(W, x1, x2, y if act == "relu" else None)
        ctx.meta = (Wg, bg, act, res is not None, rscale, rps, tap, dgrad_tap)
        return y

    @staticmethod
    def backward(ctx, dy):
        W, x1, x2, y = ctx.saved_tensors
        Wg, bg, act, has_res, rscale, rps, tap, dgrad_tap = ctx.meta
        dy = _c(dy)
        G, M, N = dy.shape
        dres = dy if has_res else None
        dz = dy
        if rscale is not None:
            # the DropPath-scaled gradient, written by the consumer norm's backward when it
            # could (GradTap), else one scaling pass
            dz = tap.take(dy) if tap is not None else None
            if dz is None:
                dz = K.scale_samples(dy, rscale, rps * N)
        if act == "relu":
            dz = K.act_bwd(dz, y, "relu")
        k1 = x1.shape[-1]
        dx1 = dx2 = None
        if dgrad_tap is not None and ctx.needs_input_grad[9] and dz.is_contiguous():
            # the producer of x1 computes this input gradient inside its own backward launch
            # (the consumer norm's LayerNorm backward in the dgrad epilogue, cmx_gemm_ln_bwd)
            dgrad_tap.put((dz, W[:, :, :k1]))
        elif ctx.needs_input_grad[9]:
            dx1 = _dgrad(dz, W[:, :, :k1], torch.empty_like(x1))
        if x2 is not None and ctx.needs_input_grad[10]:
            dx2 = _dgrad(dz, W[:, :, k1:], torch.empty_like(x2))
        _wgrad_into(dz, x1, Wg[:, :, :k1], bg)
        if x2 is not None:
            _wgrad_into(dz, x2, Wg[:, :, k1:])
        return (None, None, None, None, None, None, dres, None, None, dx1, dx2, None, None, None)


class LNTail:
    """A LayerNorm computed inside the launch that produced its input (cmx_gemm_ln): the
    producing GLinear fills ``pre`` = (y, mean, rstd), and the norm's layernorm_res consumes it
    instead of launching ln_fwd (None: not eligible, the norm launches as usual)."""
    __slots__ = ("mod", "pre")

    def __init__(self, mod):
        self.mod, self.pre = mod, None


def glinear(store, wp, bp, x1, x2=None, act="none", res=None, rscale=None, rps=1, tap=None, ln_tail=None,
            dgrad_tap=None):
    """Grouped linear using parameter ``wp`` (and bias ``bp``) of the store; x2 = second
    input segment (cat-free), res/rscale/rps = fused DropPath residual (rps = rows per sample).
    ln_tail (LNTail of the norm that consumes the output): that LayerNorm runs in this launch."""
    W = store.w(wp)
    Wg = store.g(wp)
    G = W.shape[0]
    W = W.view(G, W.shape[1], -1)
    Wg = Wg.view(G, Wg.shape[1], -1)
    b = bg = None
    if bp is not None:
        b = store.w(bp, compute=False).view(G, -1)
        bg = store.g(bp).view(G, -1)
    ln = None
    N = W.shape[1]
    if ln_tail is not None and LN_ROW and N <= 128 and N % 8 == 0:
        m = ln_tail.mod
        ln = (store.w(m.weight, compute=False).view(G, -1), store.w(m.bias, compute=False).view(G, -1), m.eps, ln_tail)
    return GLinear.apply(W, Wg, b, bg, wp, act, res, rscale, rps, x1, x2, tap, ln, dgrad_tap)


# CMX_LN_ROW=0: every LayerNorm forward as its own launch (A/B switch).  Default: a residual
# Linear whose output row fits one GEMM tile (C <= 128: stages 1-2) normalises it in its epilogue
# (cmx_gemm_ln, tail = 2): bit-identical statistics, no tickets, no second pass over the rows
LN_ROW = os.environ.get("CMX_LN_ROW", "1") != "0"

# CMX_MULTI_GEMM=0 launches the grouped Linears of GLinearMulti one by one (A/B switch)
MULTI_GEMM = os.environ.get("CMX_MULTI_GEMM", "1") != "0"


def _gemm_group(jobs):
    """Run independent K.gemm problems (kwargs dicts): the ones eligible for a multi launch
    (16-bit, 64 x 64 tiles, no split-K) as ONE cmx_gemm_multi grid, the rest one by one."""
    rest = jobs
    if MULTI_GEMM and len(jobs) > 1:
        plans = [K.gemm(**j, plan=True) for j in jobs]
        ok = [p for p in plans if p is not None]
        if len(ok) > 1:
            for i in range(0, len(ok), 4):
                if len(ok[i:i + 4]) > 1:
                    K.gemm_multi(ok[i:i + 4])
                else:
                    K.gemm(**jobs[plans.index(ok[i])])
            rest = [j for j, p in zip(jobs, plans) if p is None]
    for j in rest:
        K.gemm(**j)


class GLinearMulti(Function):
    """Independent Linears y_i = x_i W_i^T + b_i (G groups each) whose forward GEMMs run as ONE
    multi launch and whose input gradients as another: Attention.q beside Attention.kv
    (dual_segformer.py:114-121, both reading norm1's output or its spatial reduction) and the
    decoder's linear_c1..c4 (MLPDecoder.py:66-73).  Weight gradients are queued as GLinear's."""

    @staticmethod
    def forward(ctx, spec, *ts):
        n = len(spec)
        xs = ts[n:]
        ys, jobs = [], []
        for (W, Wg, b, bg), x in zip(spec, xs):
            y = torch.empty(W.shape[0], x.shape[1], W.shape[1], dtype=x.dtype, device=x.device)
            jobs.append(dict(A=x, B=W, C=y, bias=b))
            ys.append(y)
        _gemm_group(jobs)
        ctx.spec = spec
        ctx.save_for_backward(*xs)
        return tuple(ys)

    @staticmethod
    def backward(ctx, *dys):
        xs = ctx.saved_tensors
        spec = ctx.spec
        n = len(spec)
        dxs, jobs = [None] * n, []
        for i, ((W, Wg, b, bg), x, dy) in enumerate(zip(spec, xs, dys)):
            if dy is None:
                continue
            dy = _c(dy)
            if ctx.needs_input_grad[1 + n + i]:
                dxs[i] = torch.empty_like(x)
                jobs.append(dict(A=dy, B=W.transpose(1, 2), C=dxs[i]))
            _wgrad_into(dy, x, Wg, bg)
        _gemm_group(jobs)
        return (None,) * (1 + n) + tuple(dxs)


def glinear_multi(store, specs):
    """[(weight param, bias param or None, x (G, M_i, K_i))] -> the Linears' outputs (G, M_i, N_i),
    forward and input gradients each as one multi launch (GLinearMulti)."""
    spec, anchors, xs = [], [], []
    for wp, bp, x in specs:
        W = store.w(wp)
        G = W.shape[0]
        W = W.view(G, W.shape[1], -1)
        Wg = store.g(wp).view(G, W.shape[1], -1)
        b = bg = None
        if bp is not None:
            b = store.w(bp, compute=False).view(G, -1)
            bg = store.g(bp).view(G, -1)
        spec.append((W, Wg, b, bg))
        anchors.append(wp)
        xs.append(x)
    return GLinearMulti.apply(tuple(spec), *anchors, *xs)


# ---------------------------------------------------------------------------- LayerNorm
class GradTap:
    """Side channel from a norm's backward to the backward of the residual-branch GEMM that
    produced the norm's input (Block: x1 = x + drop_path(proj(o)) -> norm2(x1),
    dual_segformer.py:168-169): the norm's backward kernel also writes the DropPath-scaled
    gradient s[sample] * dx1, which the GEMM's backward uses as its dz (no scaling pass)."""
    __slots__ = ("t",)

    def __init__(self):
        self.t = None

    def put(self, t):
        self.t = t

    def take(self, like):
        t, self.t = self.t, None
        return t if (t is not None and t.shape == like.shape) else None


class LayerNormResF(Function):
    """y = LN(x), plus x passed through as a second output for a residual add downstream:
    the backward then receives both gradients and sums them in the LN backward kernel
    (cmx_layernorm_bwd_res) instead of autograd adding them.  ``scale``/``tap``: also emit
    scale[sample] * dx for the producer of x (GradTap)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, gg, bg, eps, G, scale, rps, tap, anchor, pre=None, dtap=None):
        if pre is not None:                  # computed by the producing launch (LNTail)
            y, mean, rstd = pre
        else:
            y, mean, rstd = K.layernorm_fwd(x, gamma, beta, eps, G=G)
        ctx.save_for_backward(x, gamma, mean, rstd)
        ctx.meta = (gg, bg, G, scale, rps, tap, dtap)
        ctx.set_materialize_grads(False)     # unused outputs arrive as None, not zero-filled tensors
        # y twice (a view for the second consumer, so its gradient arrives separately) and x
        return y, y.view_as(y), x

    @staticmethod
    def backward(ctx, dy, dy2, dres):
        x, gamma, mean, rstd = ctx.saved_tensors
        gg, bg, G, scale, rps, tap, dtap = ctx.meta
        C = x.shape[-1]
        R = x.numel() // C // G
        handed = dtap.take() if dtap is not None else None
        if handed is not None:
            # the consumer Linear handed over (dz, W) instead of launching its dgrad: dy = dz W and
            # this norm's backward run as ONE launch (cmx_gemm_ln_bwd, dy never stored)
            other = dy if dy is not None else dy2
            other = _c(other) if other is not None else None
            dres_c = _c(dres) if dres is not None else None
            dxs = torch.empty_like(x) if (tap is not None and scale is not None) else None
            sc = scale if dxs is not None else None
            if len(handed) == 3:             # a patchify conv's (dy, W, geometry): Attention.sr
                dyc, Wc, pg = handed
                Gc, NIg, H, Wd_, Cc = pg[:5]
                xv = x.view(Gc * NIg, H, Wd_, Cc)
                out = K.conv_patch_dgrad_ln_bwd(dyc, Wc, pg, xv, gamma, mean, rstd,
                                                dres=dres_c.view_as(xv) if dres_c is not None else None,
                                                dy2=other.view_as(xv) if other is not None else None, sscale=sc,
                                                rows_per_sample=rps, dxs=dxs.view_as(xv) if dxs is not None else None)
                if out is not None:
                    out = (out[0].view_as(x), out[1])
                else:                        # not eligible after all: the separate patch dgrad
                    dy = torch.empty(Gc * NIg, H, Wd_, Cc, dtype=dyc.dtype, device=dyc.device)
                    K.conv_patch_dgrad(dyc, Wc, dy, pg)
                    dy, dy2 = dy.view_as(x), other
            else:
                dz, Wd = handed
                out = K.gemm_ln_bwd(dz, Wd, x, gamma, mean, rstd, dres=dres_c, dy2=other, sscale=sc,
                                    rows_per_sample=rps, dxs=dxs)
                if out is None:              # not eligible after all: the separate dgrad
                    dy = _dgrad(dz, Wd, torch.empty_like(x))
                    dy2 = other
            if out is not None:
                dx, part = out
                nb = part.shape[1]
                deferred.reduce(part, gg, bg, G, nb, nb * 2 * C, 2 * C, 1, 2 * C, C, gg.stride(0), 0, bg.stride(0), 0)
                if dxs is not None:
                    tap.put(dxs)
                return dx, None, None, None, None, None, None, None, None, None, None, None, None
        elif dy is None:
            dy, dy2 = dy2, None
        dy = _c(dy) if dy is not None else torch.zeros_like(x)
        dy2 = _c(dy2) if dy2 is not None else None
        dres = _c(dres) if dres is not None else None
        dxs = torch.empty_like(x) if (tap is not None and scale is not None) else None
        defer = deferred.ENABLED
        dx, part = K.layernorm_bwd_res(dy, x, gamma, mean, rstd, G, None if defer else gg, None if defer else bg,
                                       dy2=dy2, dres=dres, sscale=scale, rows_per_sample=rps, dxs=dxs)
        if defer:
            nb = part.shape[1]
            deferred.reduce(part, gg, bg, G, nb, nb * 2 * C, 2 * C, 1, 2 * C, C, gg.stride(0), 0, bg.stride(0), 0)
        if dxs is not None:
            tap.put(dxs)
        return dx, None, None, None, None, None, None, None, None, None, None, None, None


# CMX_LN_BWD_FUSE=0: the LayerNorm backward as its own launch after the consumer's dgrad (A/B switch)
LN_BWD_FUSE = os.environ.get("CMX_LN_BWD_FUSE", "1") != "0"


def ln_bwd_fusable(x, patch=None) -> bool:
    """The consumer Linear's dgrad can carry this norm's backward (cmx_gemm_ln_bwd): 16-bit,
    C <= 128 (a dgrad tile spans the row), partials into the deferred reduce.  patch = (H, W, R):
    the consumer is a non-overlapping R x R patchify conv (Attention.sr) on an H x W grid
    (cmx_conv_patch_dgrad_ln_bwd: C 64 / 128, exact patches)."""
    C = x.shape[-1]
    ok = (LN_BWD_FUSE and deferred.ENABLED and x.dtype in (torch.bfloat16, torch.float16) and C <= 128
          and C % 8 == 0 and x.is_contiguous())
    if ok and patch is not None:
        H, W, R = patch
        ok = C in (64, 128) and H % R == 0 and W % R == 0
    return ok


def layernorm_res(store, mod, x, G, scale=None, rps=1, tap=None, tail=None, dtap=None):
    """(LN(x), LN(x) for a second consumer, x) with the fused backward (LayerNormResF).
    tail: the LNTail whose producing launch already normalised x (its pre is used if set).
    dtap: the DgradTap the consumer Linear hands its (dz, W) to (backward as one launch)."""
    gamma = store.w(mod.weight, compute=False).view(G, -1)
    beta = store.w(mod.bias, compute=False).view(G, -1)
    gg = store.g(mod.weight).view(G, -1)
    bg = store.g(mod.bias).view(G, -1)
    pre = None
    if tail is not None:
        assert tail.mod is mod
        pre, tail.pre = tail.pre, None
    return LayerNormResF.apply(x, gamma, beta, gg, bg, mod.eps, G, scale, rps, tap, mod.weight, pre, dtap)


class LayerNormF(Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, gg, bg, eps, G, anchor):
        y, mean, rstd = K.layernorm_fwd(x, gamma, beta, eps, G=G)
        ctx.save_for_backward(x, gamma, mean, rstd)
        ctx.gg, ctx.bg, ctx.G = gg, bg, G
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, mean, rstd = ctx.saved_tensors
        if deferred.ENABLED:
            dx = _layernorm_bwd_deferred(_c(dy), x, gamma, mean, rstd, ctx.G, ctx.gg, ctx.bg)
        else:
            dx = K.layernorm_bwd(_c(dy), x, gamma, mean, rstd, ctx.G, ctx.gg, ctx.bg)
        return dx, None, None, None, None, None, None, None


def _layernorm_bwd_deferred(dy, x, gamma, mean, rstd, G, gg, bg):
    """dx now; dgamma / dbeta partials (G, nb, 2C) reduced by the segment's grouped reduce."""
    C = x.shape[-1]
    dx, part = K.layernorm_bwd(dy, x, gamma, mean, rstd, G, None, None)
    nb = part.shape[1]
    deferred.reduce(part, gg, bg, G, nb, nb * 2 * C, 2 * C, 1, 2 * C, C, gg.stride(0), 0, bg.stride(0), 0)
    return dx


def layernorm(store, mod, x, G):
    gamma = store.w(mod.weight, compute=False).view(G, -1)
    beta = store.w(mod.bias, compute=False).view(G, -1)
    gg = store.g(mod.weight).view(G, -1)
    bg = store.g(mod.bias).view(G, -1)
    return LayerNormF.apply(x, gamma, beta, gg, bg, mod.eps, G, mod.weight)


# ---------------------------------------------------------------------------- split
class SplitF(Function):
    """(t[..., :k] along ``dim``, the rest) as views (CrossPath's chunk(2, dim=-1),
    net_utils.py:275-276; the modality pair o[0], o[1]); the backward concatenates the two
    gradients in one pass instead of autograd's zero-fill + slice-copy per view."""

    @staticmethod
    def forward(ctx, t, k, dim):
        ctx.k, ctx.dim, ctx.n = k, dim, t.shape[dim]
        ctx.set_materialize_grads(False)
        return t.narrow(dim, 0, k), t.narrow(dim, k, t.shape[dim] - k)

    @staticmethod
    def backward(ctx, g1, g2):
        if g1 is None and g2 is None:
            return None, None, None
        ref = g1 if g1 is not None else g2
        shp = list(ref.shape)
        if g1 is None:
            shp[ctx.dim] = ctx.k
            g1 = torch.zeros(shp, dtype=ref.dtype, device=ref.device)
        if g2 is None:
            shp[ctx.dim] = ctx.n - ctx.k
            g2 = torch.zeros(shp, dtype=ref.dtype, device=ref.device)
        return torch.cat([g1, g2], ctx.dim), None, None


def split(t, k, dim=-1):
    return SplitF.apply(t, k, dim % t.dim())


# ---------------------------------------------------------------------------- residual
class ResidualF(Function):
    """x + drop_path(y): timm DropPath as a per-sample scale (0 or 1/keep) fused in the add."""

    @staticmethod
    def forward(ctx, x, y, scale, nps):
        ctx.scale, ctx.nps = scale, nps
        return K.residual_add(x, y, scale, n_per_sample=nps)

    @staticmethod
    def backward(ctx, dout):
        dout = _c(dout)
        dy = dout if ctx.scale is None else K.scale_samples(dout, ctx.scale, ctx.nps)
        return dout, dy, None, None


class ReluF(Function):
    @staticmethod
    def forward(ctx, x):
        y = K.act_fwd(x, "relu")
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        return K.act_bwd(_c(dy), y, "relu")


# ---------------------------------------------------------------------------- attention
class SRAttentionF(Function):
    """softmax(q k^T d^-1/2) v of Attention.forward (dual_segformer.py:119-134)."""

    @staticmethod
    def forward(ctx, q, kv, Bt, N, Nk, heads, D):
        C = heads * D
        o, lse = K.sra_attn_fwd(q, kv, kv[..., C:], Bt, N, Nk, heads, D, D ** -0.5, C, 2 * C)
        o = o.view(q.shape)
        ctx.save_for_backward(q, kv, o, lse)
        ctx.dims = (Bt, N, Nk, heads, D)
        return o

    @staticmethod
    def backward(ctx, do):
        q, kv, o, lse = ctx.saved_tensors
        Bt, N, Nk, heads, D = ctx.dims
        C = heads * D
        dq, dkv = K.sra_attn_bwd(q, kv, kv[..., C:], o, _c(do), lse, Bt, N, Nk, heads, D, D ** -0.5, C, 2 * C)
        return dq.view(q.shape), dkv.view(kv.shape), None, None, None, None, None


class ActF(Function):
    """Elementwise activation with the pre-activation saved for the backward: the GELU of
    ImprovedCrossPath.act1/2 (net_utils.py:288-293, 301-302) and ImprovedChannelWeights
    (:42), on tensors a GEMM epilogue cannot keep (its pre-activation is needed later)."""

    @staticmethod
    def forward(ctx, z, act):
        ctx.act = act
        ctx.save_for_backward(z)
        return K.act_fwd(z, act)

    @staticmethod
    def backward(ctx, dy):
        (z,) = ctx.saved_tensors
        return K.act_bwd(_c(dy), z, ctx.act), None


class CrossFlashAttnF(Function):
    """ImprovedCrossAttention's core (net_utils.py:236-257) on grouped tensors q (2, M, C) and
    kv (2, M, 2C), M = B * N: o_g = softmax(q_g k_{1-g}^T d^-1/2) v_{1-g} (attn_drop p = 0), full
    token-to-token attention (Nk = N, no spatial reduction).  The SRA flash kernels run it with
    the OTHER modality's keys / values, one launch per direction (forward and backward)."""

    @staticmethod
    def forward(ctx, q, kv, B, N, heads, D):
        G, M, C = q.shape
        assert G == 2 and M == B * N and kv.shape == (2, M, 2 * C) and q.is_contiguous() and kv.is_contiguous()
        dt = K.dtype_code(q)
        o = torch.empty_like(q)
        lse = torch.empty(2, B, heads, N, dtype=torch.float32, device=q.device)
        for g in range(2):
            src = kv[1 - g]
            K.call("cmx_sra_attn_fwd", q[g], src, src[:, C:], o[g], lse[g], B, N, N, heads, D, C, 2 * C, C, D ** -0.5,
                   dt)
        ctx.save_for_backward(q, kv, o, lse)
        ctx.dims = (B, N, heads, D)
        return o

    @staticmethod
    def backward(ctx, do):
        q, kv, o, lse = ctx.saved_tensors
        B, N, heads, D = ctx.dims
        C = heads * D
        do = _c(do)
        dt = K.dtype_code(q)
        dq = torch.empty_like(q)
        dkv = torch.empty_like(kv)
        ws = K._ws(K.query("cmx_sra_attn_bwd_workspace", B, N, N, heads, D), q.device)
        for g in range(2):
            src, dsrc = kv[1 - g], dkv[1 - g]
            K.call("cmx_sra_attn_bwd", q[g], src, src[:, C:], o[g], do[g], lse[g], dq[g], dsrc, dsrc[:, C:], ws, B, N,
                   N, heads, D, C, 2 * C, C, C, C, 2 * C, D ** -0.5, dt)
        return dq, dkv, None, None, None, None


def _rowln(x, g, b, eps):
    R, C = x.shape
    y = torch.empty_like(x)
    mean = torch.empty(R, dtype=torch.float32, device=x.device)
    rstd = torch.empty_like(mean)
    K.call("cmx_rowln_fwd", x, g, b, y, mean, rstd, R, C, float(eps))
    return y, mean, rstd


def _rowln_bwd(dy, x, g, mean, rstd, gg, gb):
    R, C = x.shape
    dx = torch.empty_like(x)
    K.call("cmx_rowln_bwd", dy, x, g, mean, rstd, dx, gg, gb, R, C)
    return dx


class IFRMF(Function):
    """ImprovedFeatureRectifyModule (net_utils.py:155-180) up to its LayerNorm, on x (2, B, N, C)
    with the spatial logits sw (B*N, 2) (ImprovedSpatialWeights' conv3 output, computed by the
    caller's GEMM / BatchNorm chain):
      ImprovedChannelWeights (:33-66): avg || max pool -> Linear -> LN -> GELU -> Linear -> LN
        -> y * sigmoid(gate(y)), on (B, 4C) / (B, 2C) fp32 vectors (cmx_frm_pool_*,
        cmx_small_linear_*, cmx_layernorm_*, cmx_act_*, cmx_mul2*);
      the rectification with the learnable lambdas and un-squashed sw (cmx_ifrm_combine_*).
    The lambdas are in neither of group_weight's groups (init_func.py:33-57 only collects
    Linear / Conv / norm parameters), so the reference's optimizer never updates them: their
    gradients are computed, the fused AdamW leaves them alone (ParamStore frozen slots)."""

    @staticmethod
    def forward(ctx, x, sw, prm, anchor):
        (W1, b1, g1, e1, W3, b3, g4, e4, Wg, bgt, lc, ls, eps1, eps4) = prm["w"]
        G, B, N, C = x.shape
        dt = K.dtype_code(x)
        pooled, argmax = K.frm_pool_fwd(x, pool_tickets(anchor, x, B, C))
        h1 = K.small_linear_fwd(pooled, W1, b1, 4 * C)
        n1, m1, r1 = _rowln(h1, g1, e1, eps1)
        a1 = K.act_fwd(n1, "gelu")
        h2 = K.small_linear_fwd(a1, W3, b3, 2 * C)
        y, m2, r2 = _rowln(h2, g4, e4, eps4)
        gt = K.small_linear_fwd(y, Wg, bgt, 2 * C, "sigmoid")
        cw = torch.empty(B, 2 * C, dtype=torch.float32, device=x.device)
        K.call("cmx_mul2", y, gt, cw, B * 2 * C)
        out = torch.empty_like(x)
        K.call("cmx_ifrm_combine_fwd", x, cw, sw, lc, ls, out, B, N, C, dt)
        ctx.save_for_backward(x, sw, pooled, argmax, h1, m1, r1, n1, a1, h2, m2, r2, y, gt, cw)
        ctx.prm = prm
        return out

    @staticmethod
    def backward(ctx, dout):
        x, sw, pooled, argmax, h1, m1, r1, n1, a1, h2, m2, r2, y, gt, cw = ctx.saved_tensors
        (W1, b1, g1, e1, W3, b3, g4, e4, Wg, bgt, lc, ls, eps1, eps4) = ctx.prm["w"]
        (gW1, gb1, gg1, ge1, gW3, gb3, gg4, ge4, gWg, gbg, glc, gls) = ctx.prm["g"]
        G, B, N, C = x.shape
        dt = K.dtype_code(x)
        f32 = dict(dtype=torch.float32, device=x.device)
        dout = _c(dout)
        dx = torch.empty_like(x)
        dsw = torch.empty_like(sw)
        nb = K.query("cmx_ifrm_combine_nblk", B, N)
        part = torch.empty(nb, 2 * C, **f32)
        lpart = torch.empty(2, nb, **f32)
        K.call("cmx_ifrm_combine_bwd", dout, x, cw, sw, lc, ls, dx, dsw, part, lpart, B, N, C, dt)
        K.partials_sum(lpart[0], glc, 1, nb, 1)
        K.partials_sum(lpart[1], gls, 1, nb, 1)
        dcw = K.partials_sum(part, torch.empty(B, 2 * C, **f32), B, nb // B, 2 * C)
        # cw = y * gt, gt = sigmoid(y Wg^T + bg)
        dy = torch.empty_like(y)
        dgt = torch.empty_like(gt)
        K.call("cmx_mul2_bwd", dcw, y, gt, dy, dgt, B * 2 * C)
        dyp = K.small_linear_bwd(dgt, 1, 0, 2 * C, gt, y, Wg, gWg, gbg, 2 * C, "sigmoid")
        K.partials_sum(dyp, dy, 1, dyp.shape[0], B * 2 * C, accumulate=True)     # dy += gate path
        dh2 = _rowln_bwd(dy, h2, g4, m2, r2, gg4, ge4)
        dap = K.small_linear_bwd(dh2, 1, 0, 2 * C, h2, a1, W3, gW3, gb3, 2 * C)
        da1 = K.partials_sum(dap, torch.empty(B, 4 * C, **f32), 1, dap.shape[0], B * 4 * C)
        dn1 = K.act_bwd(da1, n1, "gelu")
        dh1 = _rowln_bwd(dn1, h1, g1, m1, r1, gg1, ge1)
        dpp = K.small_linear_bwd(dh1, 1, 0, 4 * C, h1, pooled, W1, gW1, gb1, 4 * C)
        K.frm_pool_bwd(dpp, argmax, dx)
        return dx, dsw, None, None


# ---------------------------------------------------------------------------- depthwise
class DWConvF(Function):
    """Depthwise 3x3 + bias + act (Mix-FFN DWConv+GELU, ChannelEmbed DW+ReLU)."""

    @staticmethod
    def forward(ctx, h, w, b, wg, bg, NI, ipg, H, W, act, anchor):
        C = h.shape[-1]
        out = torch.empty_like(h)
        # LDS-tiled channel counts: also save act'(z) so the backward skips the 3x3 recompute
        tiled = C % (64 if h.dtype in (torch.bfloat16, torch.float16) else 32) == 0
        gprime = torch.empty_like(h) if tiled else None
        K.call("cmx_dwconv3x3_fwd_save", h, w, b, out, gprime, NI, ipg, H, W, C, K.ACT[act], K.dtype_code(h))
        ctx.save_for_backward(h, w, b, gprime)
        ctx.meta = (wg, bg, NI, ipg, H, W, act)
        return out

    @staticmethod
    def backward(ctx, da):
        h, w, b, gprime = ctx.saved_tensors
        wg, bg, NI, ipg, H, W, act = ctx.meta
        C = h.shape[-1]
        da = _c(da)
        G, dt = NI // ipg, K.dtype_code(h)
        dh = torch.empty_like(h) if ctx.needs_input_grad[0] else None
        nbytes = K.query("cmx_dwconv3x3_bwd_workspace", NI, ipg, H, W, C)
        ws = K._ws(nbytes, h.device)
        defer = deferred.ENABLED
        dw, db = (None, None) if defer else (wg, bg)
        if gprime is not None:
            K.call("cmx_dwconv3x3_bwd_saved", da, h, gprime, w, dh, dw, db, ws, NI, ipg, H, W, C, 0, dt)
        else:
            # the LDS-tiled backward (C % 32 == 0) keeps dz on chip; the strip path writes it
            dz = torch.empty_like(h) if C % 32 else None
            K.call("cmx_dwconv3x3_bwd", da, h, w, b, dz, dh, dw, db, ws, NI, ipg, H, W, C, K.ACT[act], 0, dt)
        if defer:       # dW / db partials (G, P, C*10) = [9 taps | bias] per channel
            P = (K.query("cmx_dwconv3x3_bwd_saved_tiles", ipg, H, W) if gprime is not None
                 else nbytes // (40 * G * C) - 1)
            deferred.reduce(ws, wg, bg, G, P, P * C * 10, C * 10, C, 10, 9, wg.stride(0), 9, bg.stride(0), 1)
        return dh, None, None, None, None, None, None, None, None, None, None


def dwconv(store, conv, h, NI, ipg, H, W, act):
    G = NI // ipg
    w = store.w(conv.weight, compute=False).view(G, -1, 9)
    b = store.w(conv.bias, compute=False).view(G, -1)
    wg = store.g(conv.weight).view(G, -1, 9)
    bg = store.g(conv.bias).view(G, -1)
    return DWConvF.apply(h, w, b, wg, bg, NI, ipg, H, W, act, conv.weight)


# CMX_MLP_FUSE (A/B switch, stages 1-2: C 64 / 128, 16-bit): bit 0 = fc1 runs inside the depthwise
# forward (cmx_mlp_fc1_dwconv_fwd), bit 1 = fc2's input gradient runs inside the depthwise backward
# (cmx_mlp_fc2_dwconv_bwd, the gradient never stored); 0 = the separate GLinear / DWConvF launches.
# Either way the results are bit-identical.
MLP_FUSE = int(os.environ.get("CMX_MLP_FUSE", "3"))


class MlpF(Function):
    """Mix-FFN as one node: y = res + rscale * (fc2(gelu(dwconv3x3(fc1(x))))), i.e. GLinear ->
    DWConvF -> GLinear with the middle hand-overs inside (dual_segformer.py:67-74, 168-169).  fc1's
    backward (dgrad_tap / deferred wgrad) and fc2's forward (residual, DropPath scale, LN tail) and
    deferred wgrad are GLinear's; ``fuse`` = the MLP_FUSE bits in force."""

    @staticmethod
    def forward(ctx, x, res, W1, Wg1, b1, bg1, dw_w, dw_b, dw_wg, dw_bg, W2, Wg2, b2, bg2, a1, a2, a3, geom, rscale,
                rps, tap, ln, dgrad_tap, fuse):
        NI, ipg, H, Wd = geom
        G, M, C = x.shape
        hidden = W1.shape[1]
        dt = K.dtype_code(x)
        f0 = torch.empty(G, M, hidden, dtype=x.dtype, device=x.device)
        f = torch.empty_like(f0)
        gprime = torch.empty_like(f0)
        if fuse & 1:
            K.call("cmx_mlp_fc1_dwconv_fwd", x, W1, b1, dw_w, dw_b, f0, f, gprime, NI, ipg, H, Wd, C, hidden,
                   K.ACT["gelu"], dt)
        else:
            _fwd_gemm(x, W1, b1, f0)
            K.call("cmx_dwconv3x3_fwd_save", f0, dw_w, dw_b, f, gprime, NI, ipg, H, Wd, hidden, K.ACT["gelu"], dt)
        y = torch.empty(G, M, W2.shape[1], dtype=x.dtype, device=x.device)
        pre = None
        if ln is not None:                   # the consumer LayerNorm in fc2's launch (see GLinear.forward)
            gamma, beta, eps, sink = ln
            pre = K.gemm_ln(f, W2, y, gamma, beta, eps, bias=b2, residual=res, rscale=rscale, rows_per_sample=rps)
            sink.pre = pre
        if pre is None:
            _fwd_gemm(f, W2, b2, y, res=res, rscale=rscale, rps=rps)
        ctx.save_for_backward(x, W1, f0, gprime, dw_w, f, W2)
        ctx.meta = (Wg1, bg1, dw_wg, dw_bg, Wg2, bg2, geom, res is not None, rscale, rps, tap, dgrad_tap, fuse)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, W1, f0, gprime, dw_w, f, W2 = ctx.saved_tensors
        Wg1, bg1, dw_wg, dw_bg, Wg2, bg2, geom, has_res, rscale, rps, tap, dgrad_tap, fuse = ctx.meta
        NI, ipg, H, Wd = geom
        dy = _c(dy)
        G, M, C = dy.shape
        hidden = f0.shape[-1]
        dt = K.dtype_code(x)
        dres = dy if has_res else None
        dz = dy
        if rscale is not None:               # the DropPath-scaled gradient (see GLinear.backward)
            dz = tap.take(dy) if tap is not None else None
            if dz is None:
                dz = K.scale_samples(dy, rscale, rps * C)
        dz = _c(dz)
        nbytes = K.query("cmx_dwconv3x3_bwd_workspace", NI, ipg, H, Wd, hidden)
        defer = deferred.ENABLED
        dw, db = (None, None) if defer else (dw_wg, dw_bg)
        dh = torch.empty_like(f0)
        if fuse & 2:
            _wgrad_into(dz, f, Wg2, bg2)
            ws = K._ws(nbytes, x.device)
            K.call("cmx_mlp_fc2_dwconv_bwd", dz, W2, f0, gprime, dw_w, dh, dw, db, ws, NI, ipg, H, Wd, C, hidden, 0, dt)
        else:
            da = _dgrad(dz, W2, torch.empty_like(f))
            _wgrad_into(dz, f, Wg2, bg2)
            ws = K._ws(nbytes, x.device)
            K.call("cmx_dwconv3x3_bwd_saved", da, f0, gprime, dw_w, dh, dw, db, ws, NI, ipg, H, Wd, hidden, 0, dt)
        if defer:
            P = K.query("cmx_dwconv3x3_bwd_saved_tiles", ipg, H, Wd)
            deferred.reduce(ws, dw_wg, dw_bg, G, P, P * hidden * 10, hidden * 10, hidden, 10, 9, dw_wg.stride(0), 9,
                            dw_bg.stride(0), 1)
        dx = None
        if dgrad_tap is not None and ctx.needs_input_grad[0]:
            dgrad_tap.put((dh, W1))          # the producing norm's backward runs this dgrad (see GLinear.backward)
        elif ctx.needs_input_grad[0]:
            dx = _dgrad(dh, W1, torch.empty_like(x))
        _wgrad_into(dh, x, Wg1, bg1)
        return (dx, dres) + (None,) * 22


def mlp_fusable(x, W1, b1, W2) -> bool:
    """Block's Mix-FFN can run as MlpF: MLP_FUSE set, 16-bit, C 64 / 128 (stages 1-2), hidden in
    64-channel blocks, operands as the entry points read them (contiguous)."""
    C, hidden = x.shape[-1], W1.shape[1]
    return (MLP_FUSE & 3 != 0 and x.dtype in (torch.bfloat16, torch.float16) and C in (64, 128) and hidden % 64 == 0
            and b1 is not None and x.is_contiguous() and W1.is_contiguous() and b1.is_contiguous()
            and W2.is_contiguous() and tuple(W2.shape[1:]) == (C, hidden))


def mlp(store, m, x, NI, ipg, H, W, res=None, rscale=None, rps=1, tap=None, ln_tail=None, dgrad_tap=None):
    """Block's Mix-FFN (fc1 -> DWConv + GELU -> fc2 with the residual) on x; the arguments are those
    of the glinear / dwconv calls it stands for.  Stages 1-2 run as MlpF, the rest as those calls."""
    G = x.shape[0]

    def lin(layer):
        W, Wg = store.w(layer.weight), store.g(layer.weight)
        return (W.view(G, W.shape[1], -1), Wg.view(G, Wg.shape[1], -1), store.w(layer.bias, compute=False).view(G, -1),
                store.g(layer.bias).view(G, -1))

    W1, Wg1, b1, bg1 = lin(m.fc1)
    W2, Wg2, b2, bg2 = lin(m.fc2)
    if not mlp_fusable(x, W1, b1, W2):
        f = glinear(store, m.fc1.weight, m.fc1.bias, x, dgrad_tap=dgrad_tap)
        f = dwconv(store, m.dwconv.dwconv, f, NI, ipg, H, W, "gelu")
        return glinear(store, m.fc2.weight, m.fc2.bias, f, res=res, rscale=rscale, rps=rps, tap=tap, ln_tail=ln_tail)
    conv = m.dwconv.dwconv
    dw_w = store.w(conv.weight, compute=False).view(G, -1, 9)
    dw_b = store.w(conv.bias, compute=False).view(G, -1)
    dw_wg = store.g(conv.weight).view(G, -1, 9)
    dw_bg = store.g(conv.bias).view(G, -1)
    ln = None
    N = W2.shape[1]
    if ln_tail is not None and LN_ROW and N <= 128 and N % 8 == 0:
        nm = ln_tail.mod
        ln = (store.w(nm.weight, compute=False).view(G, -1), store.w(nm.bias, compute=False).view(G, -1), nm.eps,
              ln_tail)
    return MlpF.apply(x, res, W1, Wg1, b1, bg1, dw_w, dw_b, dw_wg, dw_bg, W2, Wg2, b2, bg2, m.fc1.weight,
                      conv.weight, m.fc2.weight, (NI, ipg, H, W), rscale, rps, tap, ln, dgrad_tap, MLP_FUSE)


class DgradTap:
    """Side channel from a GLinear's backward to the producer of its input: (dz, W) handed over
    instead of the GLinear launching dx = dz W itself (the producing norm's backward runs that
    dgrad with the LayerNorm backward in its epilogue)."""
    __slots__ = ("t",)

    def __init__(self):
        self.t = None

    def put(self, t):
        self.t = t

    def take(self):
        t, self.t = self.t, None
        return t


# ---------------------------------------------------------------------------- conv (implicit GEMM / im2col + GEMM)
# CMX_IMPLICIT_CONV=0 restores the materialised-im2col forward (A/B switch for measurements)
IMPLICIT_CONV = os.environ.get("CMX_IMPLICIT_CONV", "1") != "0"
# CMX_PE1_DIRECT=0 restores the stage-1 im2col + GEMM path (A/B switch for measurements)
PE1_DIRECT = os.environ.get("CMX_PE1_DIRECT", "1") != "0"
# CMX_CONV_DGRAD_IMPLICIT=0: a conv that asks for the im2col-free input gradient (ConvF's dgrad_implicit, the
# UPerNet head's 3x3 convs) takes the dcols + col2im path all the same (A/B switch for measurements)
CONV_DGRAD_IMPLICIT = os.environ.get("CMX_CONV_DGRAD_IMPLICIT", "1") != "0"


def _conv_dgrad_implicit(dy, W, geom):
    """The input gradient of a stride-1 'same' convolution (odd KH == KW, pad = (K - 1) / 2) without the dcols buffer:
    dx is itself such a convolution of dy with the flipped, transposed weights (cmx_conv_flip_weight), so it is ONE
    cmx_conv_implicit_fwd launch that accumulates every tap and channel in fp32 and rounds once (col2im rounds per
    tap).  16-bit, N % 64 == 0, C % 8 == 0 and the implicit kernel's 31-bit limits; None: not eligible."""
    G, NI, H, Wd, C, KH, KW, st, pad, Ho, Wo, nchw = geom
    N, NIg = W.shape[1], NI // G
    M, Kf = NIg * H * Wd, KH * KW * N
    if not (CONV_DGRAD_IMPLICIT and not nchw and dy.dtype in (torch.bfloat16, torch.float16) and st == 1 and KH == KW
            and KH % 2 == 1 and 2 * pad == KH - 1 and N % 64 == 0 and C % 8 == 0 and W.shape[-1] == KH * KW * C
            and M * N < 2 ** 30 and M * C < 2 ** 31 and C * Kf < 2 ** 30):
        return None
    Wf = K.conv_flip_weight(W, KH, KW, C)
    dx = torch.empty(G, M, C, dtype=dy.dtype, device=dy.device)
    dt = K.dtype_code(dy)
    sk = K.query("cmx_gemm_splitk", G, M, C, Kf, 0, dt)
    ws = K._ws(K.query("cmx_gemm_workspace", G, M, C, sk), dy.device) if sk > 1 else None
    K.call("cmx_conv_implicit_fwd", dy, Wf, dx, None, ws, G, NIg, H, Wd, N, KH, KW, 1, pad, H, Wd, C, M * N,
           Wf.stride(0), dx.stride(0), 0, sk, dt)
    return dx


class ConvF(Function):
    """Conv2d on NHWC (OverlapPatchEmbed.proj, Attention.sr; dual_segformer.py:196-197, :95-96):
    implicit GEMM (16-bit, C % 64 == 0), the direct stage-1 conv on the fp32 NCHW images
    (patch_embed1.hip), else im2col + grouped GEMM."""

    @staticmethod
    def forward(ctx, x, W, Wg, b, bg, geom, anchor, x2=None, dtap=None, dgrad_implicit=False):
        # geom: (G, NI, H, Wd, C, KH, KW, stride, pad, Ho, Wo, nchw); x2: the second image batch
        # of an NCHW input given as two tensors (x holds the first NI - len(x2) images).  dtap: the
        # DgradTap of the LayerNorm that produced x (its backward takes over the input gradient).
        # dgrad_implicit: take the input gradient through _conv_dgrad_implicit where it is eligible
        G, NI, H, Wd, C, KH, KW, st, pad, Ho, Wo, nchw = geom
        ctx.x2 = x2
        ctx.dtap = dtap
        ctx.dgrad_implicit = dgrad_implicit
        ctx.pe1 = None
        Kp = W.shape[-1]
        if IMPLICIT_CONV and not nchw and x.dtype in (torch.bfloat16, torch.float16) and C % 64 == 0 \
                and x.is_contiguous():
            # im2col-free: the GEMM's A operand is DMA'd tap by tap straight from x
            N = W.shape[1]
            NIg = NI // G
            y = torch.empty(G, NIg * Ho * Wo, N, dtype=x.dtype, device=x.device)
            M = NIg * Ho * Wo
            dt = K.dtype_code(x)
            sk = K.query("cmx_gemm_splitk", G, M, N, Kp, 0, dt)
            ws = K._ws(K.query("cmx_gemm_workspace", G, M, N, sk), x.device) if sk > 1 else None
            K.call("cmx_conv_implicit_fwd", x, W, y, b, ws, G, NIg, H, Wd, C, KH, KW, st, pad, Ho, Wo, N,
                   NIg * H * Wd * C, W.stride(0), y.stride(0), b.stride(0) if b is not None else 0, sk, dt)
            ctx.save_for_backward(x, W)
            ctx.meta = (Wg, bg, geom)
            ctx.xshape = x.shape
            ctx.implicit = True
            return y
        ctx.implicit = False
        if nchw and PE1_DIRECT and W.dtype in (torch.bfloat16, torch.float16) and deferred.ENABLED \
                and b is not None and (C, KH, KW, st, pad) == (3, 7, 7, 4, 3) and W.shape[1] <= 64 \
                and W.shape[1] % 8 == 0 and x.dtype == torch.float32 and x.is_contiguous() \
                and (x2 is None or x2.is_contiguous()):
            # stage 1: direct conv on the fp32 NCHW batches, no im2col columns (patch_embed1.hip)
            Bg = NI // G
            img1 = (x2 if x2 is not None else x[Bg:]) if G == 2 else None
            y = K.pe1_conv_fwd(x, img1, W, b, (G, Bg, C, H, Wd, KH, KW, st, pad, Ho, Wo))
            ctx.pe1 = (x, img1)
            ctx.save_for_backward(None, W)
            ctx.meta = (Wg, bg, geom)
            return y
        cols = torch.empty(G, NI // G * Ho * Wo, Kp, dtype=W.dtype, device=W.device)
        if nchw:
            if x2 is not None:          # (rgb, modal_x) as two batches: no concatenated copy
                K.call("cmx_im2col_nchw2_f32", x, x2, NI - x2.shape[0], cols, NI, C, H, Wd, KH, KW, st, pad, Ho, Wo, Kp,
                       K.dtype_code(cols))
            else:
                K.call("cmx_im2col_nchw_f32", x, cols, NI, C, H, Wd, KH, KW, st, pad, Ho, Wo, Kp, K.dtype_code(cols))
        else:
            K.im2col_nhwc(x, cols, NI, H, Wd, C, KH, KW, st, pad, Ho, Wo)
        y = _fwd_gemm(cols, W, b, torch.empty(G, cols.shape[1], W.shape[1], dtype=cols.dtype, device=cols.device))
        ctx.save_for_backward(cols, W)
        ctx.meta = (Wg, bg, geom)
        ctx.xshape = x.shape
        return y

    @staticmethod
    def backward(ctx, dy):
        cols, W = ctx.saved_tensors
        Wg, bg, geom = ctx.meta
        G, NI, H, Wd, C, KH, KW, st, pad, Ho, Wo, nchw = geom
        dy = _c(dy)
        if ctx.pe1 is not None:
            # per-workgroup (N, Kp + 1) partial slabs [dW | db], summed by the deferred grouped reduce
            _pe1_wgrad(dy, ctx.pe1, Wg, bg, (G, NI // G, C, H, Wd, KH, KW, st, pad, Ho, Wo), W.shape[1], W.shape[-1])
            return None, None, None, None, None, None, None, None, None, None
        if ctx.implicit:
            x = cols                 # the conv input (no cols were materialised)
            if not deferred.conv_wgrad(dy, x, Wg, bg, (G, NI // G, H, Wd, C, KH, KW, st, pad, Ho, Wo)):
                cols = torch.empty(G, NI // G * Ho * Wo, W.shape[-1], dtype=x.dtype, device=x.device)
                _wgrad_into(dy, K.im2col_nhwc(x, cols, NI, H, Wd, C, KH, KW, st, pad, Ho, Wo), Wg, bg)
        else:
            _wgrad_into(dy, cols, Wg, bg)
        dx = None
        if ctx.needs_input_grad[0] and ctx.dtap is not None and KH == KW == st and pad == 0 and H == Ho * st \
                and Wd == Wo * st:
            # the producing LayerNorm runs this input gradient inside its own backward launch
            # (cmx_conv_patch_dgrad_ln_bwd): hand (dy, W, patch geometry) over, return no dx
            ctx.dtap.put((dy, W, (G, NI // G, H, Wd, C, st, Ho, Wo)))
        elif ctx.needs_input_grad[0] and not nchw and KH == KW == st and pad == 0 and H // st == Ho and Wd // st == Wo:
            # non-overlapping patches (Attention.sr): col2im folded into the dgrad GEMM's epilogue
            exact = H % st == 0 and Wd % st == 0
            dx = (torch.empty if exact else torch.zeros)(NI, H, Wd, C, dtype=dy.dtype, device=dy.device)
            dx = K.conv_patch_dgrad(dy, W, dx, (G, NI // G, H, Wd, C, st, Ho, Wo)).view(ctx.xshape)
        elif ctx.needs_input_grad[0] and not nchw:
            dx = _conv_dgrad_implicit(dy, W, geom) if ctx.dgrad_implicit else None
            if dx is None:
                dcols = _dgrad(dy, W, torch.empty(G, NI // G * Ho * Wo, W.shape[-1], dtype=dy.dtype, device=dy.device))
                dx = torch.empty(NI, H, Wd, C, dtype=dy.dtype, device=dy.device)
                K.call("cmx_col2im_nhwc", dcols, dx, NI, H, Wd, C, KH, KW, st, pad, Ho, Wo, W.shape[-1],
                       K.dtype_code(dx))
            dx = dx.view(ctx.xshape)
        return dx, None, None, None, None, None, None, None, None, None


def _pe1_wgrad(dy, imgs, Wg, bg, geom, N, Kp):
    """The stage-1 conv's weight gradient: per-workgroup (N, Kp + 1) partial slabs [dW | db]
    (cmx_pe1_conv_wgrad), summed by the deferred grouped reduce.  geom as K.pe1_conv_fwd's."""
    ws = K.pe1_conv_wgrad(dy, *imgs, geom, N, Kp)
    G, nblk = ws.shape[:2]
    deferred.reduce(ws, Wg, bg, G, nblk, nblk * N * (Kp + 1), N * (Kp + 1), N, Kp + 1, Kp, Wg.stride(0),
                    Wg.stride(1), bg.stride(0), 1)


class PatchEmbed1F(Function):
    """Stage-1 OverlapPatchEmbed (dual_segformer.py:196-198,219): the 7x7 s4 conv straight from
    the fp32 NCHW batches with its LayerNorm in the same epilogue (cmx_pe1_conv_fwd), so the conv
    output is written once and never re-read in the forward.  Backward: the LayerNorm backward
    (dgamma / dbeta partials to the deferred reduce), then the conv's weight gradient as
    per-workgroup slabs summed by the same reduce (cmx_pe1_conv_wgrad).  The images need no
    gradient."""

    @staticmethod
    def forward(ctx, x, x2, W, Wg, b, bg, gamma, beta, gg, gb, eps, geom, anchor):
        G, NI, H, Wd, C, KH, KW, st, pad, Ho, Wo = geom
        Bg = NI // G
        img1 = (x2 if x2 is not None else x[Bg:]) if G == 2 else None
        y, out, mean, rstd = K.pe1_conv_fwd(x, img1, W, b, (G, Bg, C, H, Wd, KH, KW, st, pad, Ho, Wo),
                                            ln=(gamma, beta, eps))
        ctx.save_for_backward(y, gamma, mean, rstd)
        ctx.imgs = (x, img1)
        ctx.meta = (W.shape, Wg, bg, gg, gb, geom)
        return out

    @staticmethod
    def backward(ctx, dout):
        y, gamma, mean, rstd = ctx.saved_tensors
        wshape, Wg, bg, gg, gb, geom = ctx.meta
        G, NI, H, Wd, C, KH, KW, st, pad, Ho, Wo = geom
        dy = _layernorm_bwd_deferred(_c(dout), y, gamma, mean, rstd, G, gg, gb)
        _pe1_wgrad(dy, ctx.imgs, Wg, bg, (G, NI // G, C, H, Wd, KH, KW, st, pad, Ho, Wo), wshape[1], wshape[-1])
        return (None,) * 13


def patch_embed1(store, pe, x, G, NI, H, W, x2=None):
    """Stage-1 patch embed: conv + LayerNorm (PatchEmbed1F) when eligible (16-bit weights, the
    deferred weight gradients, N 32 / 64), else conv then layernorm.  Returns (out, Ho, Wo)."""
    mod = pe.proj
    KH, KW = mod.kernel_size
    C = x.shape[1]
    st, pad = pe.stride, pe.pad
    Ho, Wo = (H + 2 * pad - KH) // st + 1, (W + 2 * pad - KW) // st + 1
    Wt = store.w(mod.weight)
    N = Wt.shape[1]
    if (PE1_DIRECT and deferred.ENABLED and Wt.dtype in (torch.bfloat16, torch.float16) and mod.bias is not None
            and (C, KH, KW, st, pad) == (3, 7, 7, 4, 3) and N in (32, 64) and x.dtype == torch.float32
            and x.is_contiguous() and (x2 is None or x2.is_contiguous())):
        Wt = Wt.view(G, N, -1)
        Wg = store.g(mod.weight).view(G, N, -1)
        b = store.w(mod.bias, compute=False).view(G, -1)
        bg = store.g(mod.bias).view(G, -1)
        nm = pe.norm
        gamma = store.w(nm.weight, compute=False).view(G, -1)
        beta = store.w(nm.bias, compute=False).view(G, -1)
        gg = store.g(nm.weight).view(G, -1)
        gb = store.g(nm.bias).view(G, -1)
        geom = (G, NI, H, W, C, KH, KW, st, pad, Ho, Wo)
        out = PatchEmbed1F.apply(x, x2, Wt, Wg, b, bg, gamma, beta, gg, gb, nm.eps, geom, mod.weight)
        return out, Ho, Wo
    y, Ho, Wo = conv(store, mod, x, G, NI, H, W, C, st, pad, nchw=True, x2=x2)
    return layernorm(store, pe.norm, y, G), Ho, Wo


def conv(store, mod, x, G, NI, H, W, C, stride, pad, nchw=False, x2=None, dtap=None, dgrad_implicit=False):
    """dgrad_implicit (default off; the UPerNet head turns it on): the input gradient of a stride-1 'same' conv as one
    im2col-free launch where eligible (_conv_dgrad_implicit), the dcols + col2im path otherwise."""
    KH, KW = mod.kernel_size
    Ho = (H + 2 * pad - KH) // stride + 1
    Wo = (W + 2 * pad - KW) // stride + 1
    Wt = store.w(mod.weight)
    Wgt = store.g(mod.weight)
    Wt = Wt.view(G, Wt.shape[1], -1)
    Wgt = Wgt.view(G, Wgt.shape[1], -1)
    b = store.w(mod.bias, compute=False).view(G, -1) if mod.bias is not None else None
    bg = store.g(mod.bias).view(G, -1) if mod.bias is not None else None
    geom = (G, NI, H, W, C, KH, KW, stride, pad, Ho, Wo, nchw)
    return ConvF.apply(x, Wt, Wgt, b, bg, geom, mod.weight, x2, dtap, dgrad_implicit), Ho, Wo


# ---------------------------------------------------------------------------- FFM cross attention
def _heads(t, GB, N, heads, D, off=0):
    """(G, M, W) token rows (unit column stride, rows of stride rs, G * M rows evenly spaced)
    -> the (GB, heads, N, D) view of columns [off + h*D, off + (h+1)*D): one (image, head) pair
    per leading index, no copy."""
    G, M, W = t.shape
    rs = t.stride(1)
    assert t.stride(2) == 1 and t.stride(0) == M * rs and M == (GB // G) * N, (t.shape, t.stride(), GB, N)
    return t.as_strided((GB, heads, N, D), (N * rs, D, rs, 1), t.storage_offset() + off)


def _cross_attn_fwd(u, kv, B, N, heads, D):
    """CrossAttention forward (net_utils.py:199-214) on grouped tensors: u (G=2, M, C) is the
    query (raw, no projection), kv (2, M, 2C) = [k | v]; ctx_g = softmax_{-2}(k_g^T v_g * s),
    out_g = u_g @ ctx_{1-g}.  Every token contraction is a per-head MFMA GEMM over the
    (modality, image, head) triples (kernels.gemm_h2: the reference's d x d products, no
    block-diagonal padding): KV = k^T v (fp32), the softmax + crossing kernel, out = u @ ctx."""
    G, M, C = u.shape
    GB = G * B
    kh, vh = _heads(kv, GB, N, heads, D), _heads(kv, GB, N, heads, D, C)        # (GB, h, N, D)
    KV = torch.empty(GB, heads, D, D, dtype=torch.float32, device=u.device)
    K.gemm_h2(kh.transpose(2, 3), vh.transpose(2, 3), KV, out_mode=1)          # k_h^T v_h
    P = torch.empty(GB, heads, D, D, dtype=torch.float32, device=u.device)
    ctxT = torch.empty(GB, heads, D, D, dtype=u.dtype, device=u.device)
    K.call("cmx_ffm_ctx_fwd", KV, P, ctxT, G, B, heads, D, D ** -0.5, K.dtype_code(u))
    out = torch.empty(G, M, C, dtype=u.dtype, device=u.device)
    K.gemm_h2(_heads(u, GB, N, heads, D), ctxT, _heads(out, GB, N, heads, D))  # u_h @ ctx_h (crossed)
    return out, P, ctxT


def _cross_attn_bwd(dout, u, kv, P, ctxT, B, N, heads, D, du):
    """Backward of _cross_attn_fwd: du = dout @ ctx^T written into ``du`` (any row stride),
    dctx = u^T dout, the softmax-backward kernel, dk = v @ dA^T and dv = k @ dA into the halves
    of the returned dkv -- per head, like the forward."""
    G, M, C = u.shape
    GB = G * B
    dout = _c(dout)
    doh = _heads(dout, GB, N, heads, D)
    K.gemm_h2(doh, ctxT.transpose(2, 3), _heads(du, GB, N, heads, D))             # dout_h @ ctx_h^T
    dctx = torch.empty(GB, heads, D, D, dtype=torch.float32, device=u.device)
    K.gemm_h2(_heads(u, GB, N, heads, D).transpose(2, 3), doh.transpose(2, 3), dctx, out_mode=1)   # u_h^T dout_h
    dA = torch.empty(GB, heads, D, D, dtype=u.dtype, device=u.device)
    K.call("cmx_ffm_ctx_bwd", P, dctx, dA, G, B, heads, D, D ** -0.5, K.dtype_code(u))
    dkv = torch.empty(G, M, 2 * C, dtype=kv.dtype, device=kv.device)
    kh, vh = _heads(kv, GB, N, heads, D), _heads(kv, GB, N, heads, D, C)
    K.gemm_h2(vh, dA, _heads(dkv, GB, N, heads, D))                            # dk_h = v_h dA_h^T
    K.gemm_h2(kh, dA.transpose(2, 3), _heads(dkv, GB, N, heads, D, C))         # dv_h = k_h dA_h
    return dkv


class CrossAttentionF(Function):
    """CrossAttention.forward (net_utils.py:199-214) alone (the module test's entry point;
    the model runs it inside CrossPathF)."""

    @staticmethod
    def forward(ctx, u, kv, B, N, heads, D):
        out, P, ctxT = _cross_attn_fwd(u, kv, B, N, heads, D)
        ctx.save_for_backward(u, kv, P, ctxT)
        ctx.meta = (B, N, heads, D)
        return out

    @staticmethod
    def backward(ctx, dout):
        u, kv, P, ctxT = ctx.saved_tensors
        B, N, heads, D = ctx.meta
        du = torch.empty_like(u)
        dkv = _cross_attn_bwd(dout, u, kv, P, ctxT, B, N, heads, D, du)
        return du, dkv, None, None, None, None


def _stacked_w(store, p):
    W = store.w(p)
    return W.view(W.shape[0], W.shape[1], -1)


def _stacked_g(store, p):
    Wg = store.g(p)
    return Wg.view(Wg.shape[0], Wg.shape[1], -1)


class CrossPathF(Function):
    """FFM's CrossPath (net_utils.py:262-281) for both modalities as ONE autograd node:
    a = relu(channel_proj(x)); y, u = a.chunk(2, -1); v = CrossAttention(u, kv(u));
    e = x + end_proj(cat(y, v)).

    As separate nodes, x (read by channel_proj and the residual) and u (read by kv and the
    attention) each collected two gradients that autograd summed in extra passes, and the
    (y, u) split concatenated its two gradients in a third.  Here the backward writes dy and
    du straight into the halves of one (G, M, 2C) buffer (strided GEMM outputs), folds kv's
    dgrad into du and the residual gradient into dx through the GEMM residual epilogue
    (C = R + A W, in place), so x and u get one gradient each."""

    @staticmethod
    def forward(ctx, x, Wcp, Wgcp, bcp, bgcp, Wkv, Wgkv, Wend, Wgend, bend, bgend, B, N, heads, anchor):
        G, M, C = x.shape
        D = C // heads
        a = torch.empty(G, M, 2 * C, dtype=x.dtype, device=x.device)
        _fwd_gemm(x, Wcp, bcp, a, act="relu")
        y, u = a[..., :C], a[..., C:]
        kv = torch.empty(G, M, 2 * C, dtype=x.dtype, device=x.device)
        _fwd_gemm(u, Wkv, None, kv)
        v, P, ctxT = _cross_attn_fwd(u, kv, B, N, heads, D)
        e = torch.empty(G, M, C, dtype=x.dtype, device=x.device)
        _fwd_gemm(y, Wend, bend, e, res=x, x2=v)
        ctx.save_for_backward(x, a, kv, v, P, ctxT, Wcp, Wkv, Wend)
        ctx.meta = (Wgcp, bgcp, Wgkv, Wgend, bgend, B, N, heads, D)
        return e

    @staticmethod
    def backward(ctx, de):
        x, a, kv, v, P, ctxT, Wcp, Wkv, Wend = ctx.saved_tensors
        Wgcp, bgcp, Wgkv, Wgend, bgend, B, N, heads, D = ctx.meta
        G, M, C = x.shape
        de = _c(de)
        y, u = a[..., :C], a[..., C:]
        da = torch.empty(G, M, 2 * C, dtype=x.dtype, device=x.device)
        dy, du = da[..., :C], da[..., C:]
        # end_proj on cat(y, v): dy into the first half of da, dv apart; the residual passes de
        dv = torch.empty_like(v)
        # dy goes straight into dz's first half: ReLU'(y) applied in the epilogue (mask = y)
        _gemm_group([dict(A=de, B=Wend[:, :, :C].transpose(1, 2), C=dy, mask=y),    # one launch
                     dict(A=de, B=Wend[:, :, C:].transpose(1, 2), C=dv)])
        _wgrad_into(de, y, Wgend[:, :, :C], bgend)
        _wgrad_into(de, v, Wgend[:, :, C:])
        # attention: du (second half of da) = dout @ ctx^T per head, then += dkv @ Wkv (kv's dgrad)
        dkv = _cross_attn_bwd(dv, u, kv, P, ctxT, B, N, heads, D, du)
        # du += dkv @ Wkv, then ReLU'(u) (mask = u): da is dz = relu'(a) * da, no act_bwd pass
        K.gemm(dkv, Wkv.transpose(1, 2), du, residual=du, mask=u)
        _wgrad_into(dkv, u, Wgkv)
        # channel_proj + ReLU: dx = dz @ Wcp + de (residual epilogue)
        dz = da
        dx = torch.empty_like(x)
        K.gemm(dz, Wcp.transpose(1, 2), dx, residual=de)
        _wgrad_into(dz, x, Wgcp, bgcp)
        return (dx,) + (None,) * 14


def cross_path(store, cp, x, B, N, heads):
    w = lambda p: _stacked_w(store, p)   # noqa: E731
    g = lambda p: _stacked_g(store, p)   # noqa: E731
    G = x.shape[0]
    pj, kvm, ep = cp.channel_proj1, cp.cross_attn.kv1, cp.end_proj1
    return CrossPathF.apply(x, w(pj.weight), g(pj.weight), store.w(pj.bias, compute=False).view(G, -1),
                            store.g(pj.bias).view(G, -1), w(kvm.weight), g(kvm.weight), w(ep.weight), g(ep.weight),
                            store.w(ep.bias, compute=False).view(G, -1), store.g(ep.bias).view(G, -1), B, N, heads,
                            pj.weight)


class PairEmbedF(Function):
    """ChannelEmbed's two 1x1 convs on cat(o[0], o[1]) (net_utils.py:318-330: `residual` and
    `channel_embed[0]`) as ONE autograd node over the modality pair o (2, M, C): both read
    the same two halves, so as separate nodes each half collected two gradients (two autograd
    adds) and the pair split concatenated them (a copy).  The backward writes do[g] =
    dres @ Wres[:, gC:(g+1)C] for both g in one G = 2 GEMM (dres broadcast over g) and adds
    dt @ Wce0[:, gC:(g+1)C] through the residual epilogue, in place."""

    @staticmethod
    def forward(ctx, o, Wres, Wgres, Wce, Wgce, bce, bgce, anchor):
        _, M, C = o.shape
        res = torch.empty(1, M, C, dtype=o.dtype, device=o.device)
        t = torch.empty(1, M, Wce.shape[1], dtype=o.dtype, device=o.device)
        _gemm_group([dict(A=o[0:1], B=Wres, C=res, A2=o[1:2]),                 # one launch
                     dict(A=o[0:1], B=Wce, C=t, bias=bce, A2=o[1:2])])
        ctx.save_for_backward(o, Wres, Wce)
        ctx.meta = (Wgres, Wgce, bgce)
        return res, t

    @staticmethod
    def backward(ctx, dres, dt):
        o, Wres, Wce = ctx.saved_tensors
        Wgres, Wgce, bgce = ctx.meta
        _, M, C = o.shape
        dres, dt = _c(dres), _c(dt)
        do = torch.empty_like(o)

        def halves(W):              # (1, N, 2C) -> (2, N, C): [g] = W[:, gC:(g+1)C]
            return W[0].view(W.shape[1], 2, C).permute(1, 0, 2)
        K.gemm(dres.expand(2, M, dres.shape[2]), halves(Wres).transpose(1, 2), do)
        K.gemm(dt.expand(2, M, dt.shape[2]), halves(Wce).transpose(1, 2), do, residual=do)
        _wgrad_into(dres, o[0:1], Wgres[:, :, :C])
        _wgrad_into(dres, o[1:2], Wgres[:, :, C:])
        _wgrad_into(dt, o[0:1], Wgce[:, :, :C], bgce)
        _wgrad_into(dt, o[1:2], Wgce[:, :, C:])
        return (do,) + (None,) * 7


def pair_embed(store, ce, o):
    w = lambda p: _stacked_w(store, p)   # noqa: E731
    g = lambda p: _stacked_g(store, p)   # noqa: E731
    c0 = ce.channel_embed[0]
    return PairEmbedF.apply(o, w(ce.residual.weight), g(ce.residual.weight), w(c0.weight), g(c0.weight),
                            store.w(c0.bias, compute=False).view(1, -1), store.g(c0.bias).view(1, -1),
                            ce.residual.weight)


# ---------------------------------------------------------------------------- FRM
_POOL_TK: dict = {}


def pool_tickets(owner, x, B, C):
    """Zeroed arrival counters of one ChannelWeights pooling call site (cmx_frm_pool_tickets; K.tickets)."""
    return K.tickets(_POOL_TK, "cmx_frm_pool_tickets", owner, x, B, C)


# test hook (tests/test_config_parity.py): a dict makes FRMF's forward record each call's
# post-ReLU channel-MLP hidden activation y1 (B, 4C) under id() of its ChannelWeights mlp.0 weight,
# so a parity test can see which hidden units' ReLU decisions the GPU step took
FRM_PROBE = None


class FRMF(Function):
    """FeatureRectifyModule (net_utils.py:124-152) on x (2, B, N, C).

    Forward (5 launches): avg || max pooling as ONE launch (per-chunk partials folded by the
    last block to arrive, frm.hip pool_kernel), the two-layer channel MLP (ChannelWeights,
    :16-30), the SpatialWeights 2C -> C 1x1 conv as a cat-free GEMM, and ONE kernel for
    SpatialWeights' C -> 2 conv + sigmoid fused with the rectification.
    Backward (5-6 launches): one kernel for the rectification + spatial-head backward (dx direct
    path, dh, dcw / dw2 partials), one G = 2 dgrad GEMM adding both modality slices of the 2C -> C
    conv into dx, the channel MLP backward as one pass over each weight matrix (dz formed from
    the producer's partial slabs, dW / db written, dx left as partial slices; a separate dcw
    partial sum only where the slabs are too many to re-read per block), and the pooling
    backward summing those slices itself.
"""

    @staticmethod
    def forward(ctx, x, prm, anchor):
        (W1, b1, W2, b2, W0, b0, w2s, b2s) = prm["w"]
        G, B, N, C = x.shape
        dt = K.dtype_code(x)
        # ChannelWeights (net_utils.py:11-30): avg || max pool + both MLP GEMVs
        pooled, argmax = K.frm_pool_fwd(x, pool_tickets(anchor, x, B, C))
        y1 = K.small_linear_fwd(pooled, W1, b1, 4 * C, "relu")
        cw = K.small_linear_fwd(y1, W2, b2, 2 * C, "sigmoid")
        if FRM_PROBE is not None:
            FRM_PROBE[id(anchor)] = y1.detach().clone()
        # h = cat(x1, x2) W0^T + b0 (SpatialWeights' first 1x1 conv, net_utils.py:72-73), cat-free
        h = torch.empty(1, B * N, C, dtype=x.dtype, device=x.device)
        K.gemm(x[0].view(1, B * N, C), W0[None], h, bias=b0[None], A2=x[1].view(1, B * N, C))
        h = h[0]
        sw = torch.empty(B * N, 2, dtype=torch.float32, device=x.device)
        out = torch.empty_like(x)
        K.call("cmx_frm_combine_fwd", x, cw, h, w2s, b2s, sw, out, B, N, C, dt)
        ctx.save_for_backward(x, pooled, argmax, y1, cw, h, sw)
        ctx.prm = prm
        ctx.set_materialize_grads(False)
        # the output twice (a view for the second consumer: the FFM beside the next stage), so the
        # two gradients arrive separately and the combine backward sums them on load (no add launch)
        return out, out.view_as(out)

    @staticmethod
    def backward(ctx, dout, dout2):
        x, pooled, argmax, y1, cw, h, sw = ctx.saved_tensors
        (W1, b1, W2, b2, W0, b0, w2s, b2s) = ctx.prm["w"]
        (gW1, gb1, gW2, gb2, gW0, gb0, gw2s, gb2s) = ctx.prm["g"]
        G, B, N, C = x.shape
        dt = K.dtype_code(x)
        if dout is None:
            dout, dout2 = dout2, None
        if dout is None:
            return None, None, None
        dout = _c(dout)
        dout2 = _c(dout2) if dout2 is not None else None
        dx = torch.empty_like(x)
        dh = torch.empty_like(h)
        nb = K.query("cmx_frm_combine_bwd_nblk", N, C, dt)
        ws = K._ws(K.query("cmx_frm_combine_bwd_workspace", B, N, C, dt), x.device)
        K.call("cmx_frm_combine_bwd", dout, dout2, x, cw, sw, h, w2s, dx, dh, ws, B, N, C, dt)
        psp = ws[B * nb * 2 * C:B * nb * 2 * C + B * nb * (2 * C + 2)]
        if deferred.ENABLED:          # [dw2 | db2] partials: weight gradients, summed by the grouped reduce
            deferred.reduce(psp, gw2s, gb2s, 1, B * nb, 0, 2 * C + 2, 1, 2 * C + 2, 2 * C, 0, 0, 0, 0)
        else:
            tmp = torch.empty(2 * C + 2, dtype=torch.float32, device=x.device)
            K.partials_sum(psp, tmp, 1, B * nb, 2 * C + 2)
            gw2s.view(-1).copy_(tmp[:2 * C])
            gb2s.view(-1).copy_(tmp[2 * C:])
        # dx_g += dh @ W0[:, gC:(g+1)C] for both modalities in one launch (A = dh for both groups)
        Wd = W0.view(C, 2, C).permute(1, 0, 2)                          # (2, C_out, C_in), strides (C, 2C, 1)
        dx2 = dx.view(2, B * N, C)
        K.gemm(dh[None].expand(2, B * N, C), Wd.transpose(1, 2), dx2, residual=dx2)
        _wgrad_into(dh[None], x[0].view(1, B * N, C), gW0[None, :, :C], gb0.view(1, C))
        _wgrad_into(dh[None], x[1].view(1, B * N, C), gW0[None, :, C:])
        # channel MLP backward: dcw partial slabs (B, nb, 2C) -> W2 pass -> W1 pass -> pooling.  When
        # a W2-pass block's share of the slabs is small (B * 2C/16 values x nb slabs <= 8192: stages
        # 1-2) it sums them itself (slab q of image m at ws[q*2C + m*nb*2C]); otherwise every one
        # of its column blocks would re-read them and one partial-sum launch is cheaper
        ns = K.query("cmx_small_linear_nslice")
        if B * -(-2 * C // ns) * nb <= 8192:
            dcw, nsl, ss, sm = ws, nb, 2 * C, nb * 2 * C
        else:
            dcw, nsl, ss, sm = torch.empty(B, 2 * C, dtype=torch.float32, device=x.device), 1, 0, 2 * C
            K.partials_sum(ws, dcw, B, nb, 2 * C)
        dy1p = K.small_linear_bwd(dcw, nsl, ss, sm, cw, y1, W2, gW2, gb2, 2 * C, "sigmoid")
        dpp = K.small_linear_bwd(dy1p, ns, B * 4 * C, 4 * C, y1, pooled, W1, gW1, gb1, 4 * C, "relu")
        K.frm_pool_bwd(dpp, argmax, dx)
        return dx, None, None


def frm(store, mod, x):
    """FRMF on x (2, B, N, C): (rectified pair for the FFM, the same for the next stage)."""
    cwm, swm = mod.channel_weights.mlp, mod.spatial_weights.mlp
    C = x.shape[-1]
    f32 = lambda p: store.w(p, stacked=False, compute=False)
    cmp = lambda p: store.w(p, stacked=False)
    g = lambda p: store.g(p, stacked=False)
    prm = {
        # fp32 for the channel MLP / spatial head (VALU GEMVs and row dots in fp32);
        # compute dtype for the spatial 2C -> C GEMM
        "w": (f32(cwm[0].weight), f32(cwm[0].bias), f32(cwm[2].weight), f32(cwm[2].bias),
              cmp(swm[0].weight).view(C, 2 * C), f32(swm[0].bias), f32(swm[2].weight).view(2, C), f32(swm[2].bias)),
        "g": (g(cwm[0].weight), g(cwm[0].bias), g(cwm[2].weight), g(cwm[2].bias),
              g(swm[0].weight).view(C, 2 * C), g(swm[0].bias), g(swm[2].weight).view(2, C), g(swm[2].bias)),
    }
    return FRMF.apply(x, prm, cwm[0].weight)


# ---------------------------------------------------------------------------- BatchNorm
def sync_bn_sums(sums: torch.Tensor, count: float, group) -> float:
    """SyncBatchNorm exchange (MLPDecoder.py:53 under train.py:64-65): all-reduce the fp64
    per-channel sums over the ranks of ``group`` in place; return the global row count
    (equal per-rank batches, dataloader.py:155).  No-op without a group."""
    if group is None:
        return count
    import torch.distributed as dist
    dist.all_reduce(sums, group=group)
    return count * dist.get_world_size(group)


# local-statistics BatchNorms of at most this many rows (the stage-4 ChannelEmbed BNs: 600 rows at
# B2 480 x 640) run forward and backward as one launch each (cmx_bn_small_fwd / _bwd) instead of
# three; at 2400 rows (stage 3) the one-launch form is slower (batchnorm.hip); 0 = off
BN_SMALL_M = int(os.environ.get("CMX_BN_SMALL_M", "600"))


class BatchNormF(Function):
    @staticmethod
    def forward(ctx, x, res, prm, training, act, dscale, rps, group, anchor):
        gamma, beta, gg, bg, rm, rv, eps, momentum = prm
        M, C = x.shape
        dt = K.dtype_code(x)
        mean = torch.empty(C, dtype=torch.float32, device=x.device)
        invstd = torch.empty(C, dtype=torch.float32, device=x.device)
        count = float(M)
        ctx.small = training and group is None and M <= BN_SMALL_M and C % 16 == 0
        y = torch.empty_like(x)
        if ctx.small:
            sums = torch.empty(2, C, dtype=torch.float64, device=x.device)
            K.call("cmx_bn_small_fwd", x, res, gamma, beta, dscale, y, sums, mean, invstd, rm, rv, M, C, rps,
                   K.ACT[act], eps, momentum, dt)
        elif training:
            sums, ws = K.bn_scratch(M, C, x.device)
            if group is None:       # local statistics: the fold finalizes (no exchange in between)
                K.call("cmx_bn_stats_finalize", x, sums, ws, M, C, eps, momentum, rm, rv, mean, invstd, dt)
            else:
                K.call("cmx_bn_stats", x, sums, ws, M, C, dt)
                count = sync_bn_sums(sums, count, group)
                K.call("cmx_bn_finalize", sums, count, eps, momentum, rm, rv, mean, invstd, C, 1)
        else:
            K.call("cmx_bn_finalize", None, 1.0, eps, momentum, rm, rv, mean, invstd, C, 0)
        if not ctx.small:
            K.call("cmx_bn_apply", x, mean, invstd, gamma, beta, res, dscale, y, M, C, rps, K.ACT[act], dt)
        ctx.save_for_backward(x, res if res is not None else x, mean, invstd)
        ctx.meta = (prm, training, act, dscale, rps, group, count, res is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, res, mean, invstd = ctx.saved_tensors
        prm, training, act, dscale, rps, group, count, has_res = ctx.meta
        gamma, beta, gg, bg, rm, rv, eps, momentum = prm
        res = res if has_res else None
        M, C = x.shape
        dt = K.dtype_code(x)
        dy = _c(dy)
        dx = torch.empty_like(x)
        dres = torch.empty_like(x) if has_res else None
        if ctx.small:
            K.call("cmx_bn_small_bwd", dy, x, mean, invstd, gamma, beta, res, dscale, gg, bg, dx, dres, M, C, rps,
                   K.ACT[act], 0, dt)
            return dx, dres, None, None, None, None, None, None, None
        sums, ws = K.bn_scratch(M, C, x.device)
        K.call("cmx_bn_bwd_reduce", dy, x, mean, invstd, gamma, beta, res, dscale, sums, gg, bg, ws, M, C, rps,
               K.ACT[act], 0, dt)
        if training:
            sync_bn_sums(sums, count, group)
        K.call("cmx_bn_bwd_apply", dy, x, mean, invstd, gamma, beta, res, dscale, sums, count, dx, dres, M, C, rps,
               K.ACT[act], training, dt)
        return dx, dres, None, None, None, None, None, None, None


def batchnorm(store, bn, x, training, res=None, act="none", dscale=None, rps=1, group=None):
    prm = (store.w(bn.weight, stacked=False, compute=False), store.w(bn.bias, stacked=False, compute=False),
           store.g(bn.weight, stacked=False), store.g(bn.bias, stacked=False), bn.running_mean, bn.running_var,
           float(bn.eps), float(bn.momentum))
    if training and not getattr(bn, "_nbt_shared", False):
        bn.num_batches_tracked.add_(1)
    return BatchNormF.apply(x, res, prm, training, act, dscale, rps, group, bn.weight)


# ---------------------------------------------------------------------------- channel-attention gate
_SE_TK: dict = {}


def se_tickets(owner, x, B, C):
    """Zeroed arrival counters of one gate's pooling (cmx_se_pool_tickets; K.tickets)."""
    return K.tickets(_SE_TK, "cmx_se_pool_tickets", owner, x, B, C, least=1)


class SEGateF(Function):
    """MLPDecoderpp's channel attention + Dropout2d (MLPDecoderpp.py:55-61, 81-85) on the fused map
    y (B, N, C):  a = sigmoid(W2 GELU(W1 avgpool(y) + b1) + b2),  out = y * a * dscale.

    Forward (5 launches): the pooling (cmx_se_pool_fwd, per-chunk partials folded by the last
    block to arrive), the hidden GEMV, its GELU, the output GEMV with the sigmoid, the scale.
    Backward (7 launches): da as per-chunk slices (cmx_se_bwd_reduce) that the sigmoid layer's
    one-pass backward sums itself; its dx slices summed (cmx_partials_sum) for the GELU backward
    on the saved pre-activation (cmx_small_linear_bwd derives act' from the saved OUTPUT, which
    GELU does not allow); the hidden layer's backward; cmx_se_bwd_apply, which sums that layer's
    dx slices as the pooled gradient.  The MLP runs on the fp32 master weights; its gradients
    go straight into the flat gradient buffer."""

    @staticmethod
    def forward(ctx, y, prm, dscale, anchor):
        (W1, b1, W2, b2) = prm["w"]
        B, N, C = y.shape
        H = W1.shape[0]
        dt = K.dtype_code(y)
        pooled = torch.empty(B, C, dtype=torch.float32, device=y.device)
        ws = K._ws(K.query("cmx_se_pool_workspace", B, N, C), y.device)
        K.call("cmx_se_pool_fwd", y, pooled, ws, se_tickets(anchor, y, B, C), B, N, C, dt)
        z1 = K.small_linear_fwd(pooled, W1, b1, H)
        h1 = K.act_fwd(z1, "gelu")
        a = K.small_linear_fwd(h1, W2, b2, C, "sigmoid")
        out = torch.empty_like(y)
        K.call("cmx_se_scale_fwd", y, a, dscale, out, B, N, C, dt)
        ctx.save_for_backward(y, a, z1, pooled)
        ctx.meta = (prm, dscale)
        return out

    @staticmethod
    def backward(ctx, dout):
        y, a, z1, pooled = ctx.saved_tensors
        prm, dscale = ctx.meta
        (W1, b1, W2, b2) = prm["w"]
        (gW1, gb1, gW2, gb2) = prm["g"]
        B, N, C = y.shape
        H = W1.shape[0]
        dt = K.dtype_code(y)
        f32 = dict(dtype=torch.float32, device=y.device)
        dout = _c(dout)
        nda = K.query("cmx_se_bwd_nslice", B, N, C)
        dap = torch.empty(nda, B, C, **f32)
        K.call("cmx_se_bwd_reduce", dout, y, dscale, dap, B, N, C, dt)
        h1 = K.act_fwd(z1, "gelu")                    # GELU(z1) again: (B, C/4) values
        dh1p = K.small_linear_bwd(dap, nda, B * C, C, a, h1, W2, gW2, gb2, C, "sigmoid")
        dh1 = K.partials_sum(dh1p, torch.empty(B, H, **f32), 1, dh1p.shape[0], B * H)
        dz1 = K.act_bwd(dh1, z1, "gelu")
        dpp = K.small_linear_bwd(dz1, 1, 0, H, z1, pooled, W1, gW1, gb1, H)
        dy = torch.empty_like(y)
        K.call("cmx_se_bwd_apply", dout, a, dscale, dpp, dpp.shape[0], B * C, dy, B, N, C, dt)
        return dy, None, None, None


def se_gate(store, att, y, dscale=None):
    """SEGateF on y (B, N, C) with the head's ``attention`` Sequential (its two 1x1 convs at
    [1] and [3], MLPDecoderpp.py:57,59)."""
    f32 = lambda p: store.w(p, stacked=False, compute=False)
    g = lambda p: store.g(p, stacked=False)
    c1, c2 = att[1], att[3]
    prm = {"w": (f32(c1.weight), f32(c1.bias), f32(c2.weight), f32(c2.bias)),
           "g": (g(c1.weight), g(c1.bias), g(c2.weight), g(c2.bias))}
    return SEGateF.apply(y, prm, dscale, c1.weight)


# ---------------------------------------------------------------------------- eASPP neck
class DilatedConv3F(Function):
    """The ASPPConv 3x3 convolutions (dilation = padding = rate, dual_segformer_w_ef_aspp.py:18-28) of the three
    branches at one depth level: forward, input gradient and weight gradient each as ONE grouped launch
    (cmx_easpp_conv_*; the weight gradient folds its per-workgroup partials in a second one).  x_g (B*h*w, 64),
    Ws / Wgs: the branches' tap-major weights and their fp32 gradient views."""

    @staticmethod
    def forward(ctx, geom, Ws, Wgs, a0, a1, a2, x0, x1, x2):
        B, h, w, rates = geom
        xs = (x0, x1, x2)
        ys = tuple(torch.empty_like(x) for x in xs)
        K.easpp_conv("cmx_easpp_conv_fwd", xs, Ws, ys, B, h, w, rates)
        ctx.save_for_backward(*xs)
        ctx.meta = (geom, Ws, Wgs)
        return ys

    @staticmethod
    def backward(ctx, *dys):
        xs = ctx.saved_tensors
        (B, h, w, rates), Ws, Wgs = ctx.meta
        dys = tuple(_c(d) for d in dys)
        dxs = tuple(torch.empty_like(x) for x in xs)
        K.easpp_conv("cmx_easpp_conv_dgrad", dys, Ws, dxs, B, h, w, rates)
        K.easpp_conv_wgrad(dys, xs, Wgs, B, h, w, rates)
        return (None,) * 6 + dxs


def dilated_conv3(store, convs, xs, B, h, w):
    """DilatedConv3F on the three branches' nn.Conv2d modules ``convs`` (3x3, 64 -> 64, one dilation each)."""
    Ws = tuple(store.w(c.weight, stacked=False) for c in convs)
    Wgs = tuple(store.g(c.weight, stacked=False) for c in convs)
    geom = (B, h, w, tuple(int(c.dilation[0]) for c in convs))
    return DilatedConv3F.apply(geom, Ws, Wgs, *(c.weight for c in convs), *xs)


class PooledConvF(Function):
    """AsppPooling's AdaptiveAvgPool2d(1) and bias-free 1x1 conv (:31-45) on x (B*N, C): z (B, Cout) fp32 =
    mean_n(x) W^T on the fp32 master weight (cmx_se_pool_fwd, cmx_small_linear_fwd).  Backward: the tiny linear's
    one-pass backward (dW into the gradient buffer, dx as slices), then the pooling's adjoint, which sums the slices
    (cmx_easpp_pool_bwd)."""

    @staticmethod
    def forward(ctx, x, W, Wg, B, N, anchor):
        x = _c(x)
        C = x.shape[-1]
        pooled = torch.empty(B, C, dtype=torch.float32, device=x.device)
        ws = K._ws(K.query("cmx_se_pool_workspace", B, N, C), x.device)
        K.call("cmx_se_pool_fwd", x, pooled, ws, se_tickets(anchor, x, B, C), B, N, C, K.dtype_code(x))
        z = K.small_linear_fwd(pooled, W, None, W.shape[0])
        ctx.save_for_backward(pooled, z, W)
        ctx.meta = (Wg, B, N, x.dtype)
        return z

    @staticmethod
    def backward(ctx, dz):
        pooled, z, W = ctx.saved_tensors
        Wg, B, N, dtype = ctx.meta
        C, Cout = pooled.shape[1], W.shape[0]
        dpp = K.small_linear_bwd(_c(dz), 1, 0, Cout, z, pooled, W, Wg, None, Cout)
        dx = torch.empty(B * N, C, dtype=dtype, device=dz.device)
        K.call("cmx_easpp_pool_bwd", dpp, dpp.shape[0], B * C, dx, B, N, C, K.dtype_code(dx))
        return dx, None, None, None, None, None


def pooled_conv(store, conv, x, B, N):
    """PooledConvF with the 1x1 nn.Conv2d ``conv`` of AsppPooling.gap."""
    return PooledConvF.apply(x, store.w(conv.weight, stacked=False, compute=False),
                             store.g(conv.weight, stacked=False), B, N, conv.weight)


class EasppConcatF(Function):
    """cat[x_in, b1, b2, b3, pool] (:152) with the pooled branch's bilinear upsample of a 1x1 map, a broadcast
    (:44), in one launch: y_i (B*N, Cm), pool (B, Cm) fp32 -> (B*N, 5 Cm).  Backward, one launch: the four column
    slots and the pooled branch's sum over each image's pixels."""

    @staticmethod
    def forward(ctx, y0, y1, y2, y3, pool, B, N):
        y0, y1, y2, y3, pool = (_c(t) for t in (y0, y1, y2, y3, pool))     # the entry point takes no strides
        Cm = y0.shape[-1]
        cat = torch.empty(B * N, 5 * Cm, dtype=y0.dtype, device=y0.device)
        K.call("cmx_easpp_concat_fwd", y0, y1, y2, y3, pool, cat, B, N, Cm, K.dtype_code(y0))
        ctx.meta = (B, N, Cm)
        return cat

    @staticmethod
    def backward(ctx, dcat):
        B, N, Cm = ctx.meta
        dcat = _c(dcat)
        ds = tuple(torch.empty(B * N, Cm, dtype=dcat.dtype, device=dcat.device) for _ in range(4))
        dpool = torch.empty(B, Cm, dtype=torch.float32, device=dcat.device)
        K.call("cmx_easpp_concat_bwd", dcat, *ds, dpool, B, N, Cm, K.dtype_code(dcat))
        return (*ds, dpool, None, None)


def easpp_dropout_scale(state, n, p, device):
    """The elementwise Dropout(p) of eASPP.project as batchnorm's dscale: n fp32 values (u >= p) / (1 - p) drawn on
    the device (cmx_easpp_dropout_mask); state = (seed, (step, arrival counter) uint64 pair as int64)."""
    scale = torch.empty(n, dtype=torch.float32, device=device)
    K.call("cmx_easpp_dropout_mask", scale, n, float(p), state[0], state[1])
    return scale


# ---------------------------------------------------------------------------- DeepLabV3+ head
class AsppConv3F(Function):
    """ASPP.b1 .. b3's dilated 3x3 convolutions Cin -> Cout (deeplabv3plus.py:37-47) on ONE shared input x (B*h*w, Cin):
    forward, input gradient and weight gradient each as one grouped launch (cmx_aspp_conv_*; the weight gradient folds
    per-chunk partials in a second one when the rows are split).  The input gradient is the sum over the three
    branches, accumulated in fp32 and rounded once: autograd would otherwise add three full maps.  Ws / Wgs: the
    branches' tap-major weights and their fp32 gradient views."""

    @staticmethod
    def forward(ctx, geom, Ws, Wgs, a0, a1, a2, x):
        B, h, w, rates = geom
        if x.stride(-1) != 1:
            x = x.contiguous()
        ctx.save_for_backward(x)
        ctx.meta = (geom, Ws, Wgs)
        return K.aspp_conv_fwd(x, Ws, B, h, w, rates)

    @staticmethod
    def backward(ctx, *dys):
        x, = ctx.saved_tensors
        (B, h, w, rates), Ws, Wgs = ctx.meta
        dys = tuple(_c(d) for d in dys)
        dx = K.aspp_conv_dgrad(dys, Ws, B, h, w, rates) if ctx.needs_input_grad[6] else None
        K.aspp_conv_wgrad(dys, x, Wgs, B, h, w, rates)
        return (None,) * 6 + (dx,)


def aspp_conv3(store, convs, x, B, h, w):
    """AsppConv3F on the three branches' nn.Conv2d modules ``convs`` (3x3, one dilation each, the same Cin -> Cout)."""
    Ws = tuple(store.w(c.weight, stacked=False) for c in convs)
    Wgs = tuple(store.g(c.weight, stacked=False) for c in convs)
    geom = (B, h, w, tuple(int(c.dilation[0]) for c in convs))
    return AsppConv3F.apply(geom, Ws, Wgs, *(c.weight for c in convs), x)


class UpcatAcF(Function):
    """torch.cat([F.interpolate(lo, (H, W), mode='bilinear', align_corners=True), skip], 1) (deeplabv3plus.py:32-33) on
    token rows, one launch each way: lo (B*h*w, C), skip (B*H*W, Cs) -> (B*H*W, C + Cs)."""

    @staticmethod
    def forward(ctx, lo, skip, dims):
        B, h, w, H, W = dims
        lo, skip = _c(lo), _c(skip)
        ctx.meta = (dims, lo.shape[-1], skip.shape[-1])
        return K.upcat_ac_fwd(lo, skip, B, h, w, H, W)

    @staticmethod
    def backward(ctx, dcat):
        (B, h, w, H, W), C, Cs = ctx.meta
        dlo, dskip = K.upcat_ac_bwd(_c(dcat), B, h, w, H, W, C, Cs)
        return dlo, dskip, None


# ---------------------------------------------------------------------------- UPerNet head (include/cmx_uper.h)
class ColumnTap:
    """Side channel from UpcatMultiF's backward to PpmPoolF's: the PPM concat's gradient towards its skip columns (a
    strided view of dcat, nothing copied), which the pooling backward adds in its own launch (cmx_ppm_pool_bwd's
    ``add``).  The skip and the pooled branches are the same tensor, so autograd would otherwise add the two terms in
    a launch of its own."""
    __slots__ = ("t",)

    def __init__(self):
        self.t = None

    def put(self, t):
        self.t = t

    def take(self):
        t, self.t = self.t, None
        return t


class PpmPoolF(Function):
    """The pyramid pooling of PPM (UPernet.py:107-146): nn.AdaptiveAvgPool2d(s) of x (B*h*w, C) at up to four scales in
    one launch each way.  Returns one (B*s*s, C) block per scale, views of one (B * sum s^2, C) buffer in which scale
    k's block starts at row B * sum_{j<k} s_j^2; the backward puts the blocks' gradients back into one such buffer
    (one torch.cat of at most B * 256 rows).  tap (ColumnTap, optional): gradient rows of x handed over by the
    concat's backward, added inside the backward launch."""

    @staticmethod
    def forward(ctx, x, dims, tap=None):
        B, h, w, scales = dims
        ctx.meta = (dims, tap, x.shape[-1], x.dtype)
        return tuple(K.ppm_pool_fwd(_c(x), B, h, w, scales).split([B * s * s for s in scales]))

    @staticmethod
    def backward(ctx, *dblocks):
        (B, h, w, scales), tap, C, dtype = ctx.meta
        dev = next(d for d in dblocks if d is not None).device
        dpooled = torch.cat([d if d is not None else torch.zeros(B * s * s, C, dtype=dtype, device=dev)
                             for d, s in zip(dblocks, scales)])
        add = tap.take() if tap is not None else None
        return K.ppm_pool_bwd(dpooled, add, B, h, w, scales), None, None


class UpcatMultiF(Function):
    """torch.cat([skip, up(src_0), ..., up(src_{n-1})], 1), up = bilinear align_corners=False onto (H, W)
    (UPernet.py:58-66, :94-100), on token rows, one launch each way: skip (B*H*W, Cs), src_i (B*h_i*w_i, C) ->
    (B*H*W, Cs + n*C).  dims = (B, H, W, ((h_0, w_0), ...)).  tap (ColumnTap, optional): the gradient towards skip is
    handed over as a view of dcat instead of being copied out, and None is returned for it."""

    @staticmethod
    def forward(ctx, dims, tap, skip, *srcs):
        B, H, W, grids = dims
        skip, srcs = _c(skip), [_c(t) for t in srcs]
        ctx.meta = (dims, tap, skip.shape[-1], srcs[0].shape[-1])
        return K.upcat_multi_fwd(skip, srcs, B, H, W, grids)

    @staticmethod
    def backward(ctx, dcat):
        (B, H, W, grids), tap, Cs, C = ctx.meta
        dcat = _c(dcat)
        dskip, ds = K.upcat_multi_bwd(dcat, B, H, W, Cs, C, grids, want_skip=tap is None)
        if tap is not None:
            tap.put(dcat[:, :Cs])
        return (None, None, dskip, *ds)


class UpAddF(Function):
    """hi + up(lo), the top-down step of the FPN (UPernet.py:78-84) as an out-of-place sum: hi (B*H*W, C), lo (B*h*w, C).
    Backward: dhi is dout itself; dlo is the gather adjoint cmx_upcat_multi_bwd with no skip columns and one source
    (exact for any C, where cmx_bilinear_adjoint3 needs C % 128 == 0 in 16 bits)."""

    @staticmethod
    def forward(ctx, hi, lo, dims):
        B, h, w, H, W = dims
        ctx.meta = (dims, hi.shape[-1])
        return K.up_add_fwd(_c(hi), _c(lo), B, h, w, H, W)

    @staticmethod
    def backward(ctx, dout):
        (B, h, w, H, W), C = ctx.meta
        dout = _c(dout)
        _, (dlo,) = K.upcat_multi_bwd(dout, B, H, W, 0, C, ((h, w),), want_skip=False)
        return dout, dlo, None


# ---------------------------------------------------------------------------- decoder fuse
def _adjoint_to(dZ, B, H1, W1, h, w, E):
    """up^T dZ: the bilinear adjoint of the (h, w) -> (H1, W1) upsample, (B, h*w, E) in dZ's
    dtype (two separable 1-D gather passes, fp32 in between, no atomics)."""
    tmp = torch.empty(B * H1, w, E, dtype=torch.float32, device=dZ.device)
    K.bilinear_adjoint_1d(dZ, tmp, B * H1, W1, w, E, W1 * E, E)
    g = torch.empty(B, h * w, E, dtype=dZ.dtype, device=dZ.device)
    return K.bilinear_adjoint_1d(tmp, g, B, H1, h, w * E, H1 * w * E, w * E)


class DecoderFuseF(Function):
    """DecoderHead's upsample + concat + linear_fuse 1x1 conv (MLPDecoder.py:66-77) without the
    (B, N1, 4E) concat.  The 1x1 conv is linear and bilinear interpolation is linear with
    weights summing to 1, so for each upsampled branch  W_i up(e_i) = up(W_i e_i):

        Z = e1 W_c1^T + b + up(e4 W_c4^T) + up(e3 W_c3^T) + up(e2 W_c2^T)

    The three branch products run at their own (low) resolution and the GEMM of the c1 branch
    adds their bilinear upsample in its epilogue (cmx_decoder_fuse_fwd).  Backward: dZ feeds
    the c1 dgrad / wgrad and the bias gradient at full resolution; each upsampled branch gets
    dz_i = up^T dZ (bilinear adjoint) and then its dgrad / wgrad at low resolution.
    Executed FLOPs: 38400 x 512 x 512 + low-res products instead of 38400 x 2048 x 512 (B2, bs=2);
    the step roofline keeps the reference's op-by-op count (flops.py)."""

    # Wf column slot of the branches (c4, c3, c2, c1): the reference head concatenates [c4 | c3 | c2 | c1]
    SLOTS = (0, 1, 2, 3)

    @staticmethod
    def forward(ctx, e4, e3, e2, e1, Wf, Wfg, bf, bfg, sizes, anchor):
        return _decoder_fuse_fwd(ctx, DecoderFuseF.SLOTS, e4, e3, e2, e1, Wf, Wfg, bf, bfg, sizes)

    @staticmethod
    def backward(ctx, dZ):
        return _decoder_fuse_bwd(ctx, dZ)


class DecoderFuseC1F(DecoderFuseF):
    """DecoderFuseF for a head whose concat is [c1 | c2 | c3 | c4] (MLPDecoderpp.py:80): the same
    launches, each branch on its own column slot of the conv."""
    SLOTS = (3, 2, 1, 0)

    @staticmethod
    def forward(ctx, e4, e3, e2, e1, Wf, Wfg, bf, bfg, sizes, anchor):
        return _decoder_fuse_fwd(ctx, DecoderFuseC1F.SLOTS, e4, e3, e2, e1, Wf, Wfg, bf, bfg, sizes)


def _decoder_fuse_fwd(ctx, slots, e4, e3, e2, e1, Wf, Wfg, bf, bfg, sizes):
    B, N1, E = e1.shape
    (H1, W1), hw = sizes[0], sizes[1:]        # hw: grids of c2, c3, c4
    W = Wf[0]                                 # (E, 4E): column slots[j] of branch j of (c4, c3, c2, c1)
    zs, jobs = [], []
    for j, (e, (h, w)) in enumerate(zip((e4, e3, e2), (hw[2], hw[1], hw[0]))):
        slot = slots[j]
        z = torch.empty(1, B * h * w, E, dtype=e.dtype, device=e.device)
        jobs.append(dict(A=e.reshape(1, B * h * w, E), B=W[None, :, slot * E:(slot + 1) * E], C=z))
        zs.append(z)
    _gemm_group(jobs)                         # the three branch products: one launch
    Z = K.decoder_fuse_fwd(_c(e1), W[:, slots[3] * E:(slots[3] + 1) * E], bf, zs, H1, W1, hw)
    ctx.save_for_backward(e4, e3, e2, e1, Wf)
    ctx.meta = (Wfg, bfg, sizes, slots)
    return Z


def _decoder_fuse_bwd(ctx, dZ):
    e4, e3, e2, e1, Wf = ctx.saved_tensors
    Wfg, bfg, sizes, slots = ctx.meta
    B, N1, E = e1.shape
    (H1, W1), hw = sizes[0], sizes[1:]
    dZ = _c(dZ).view(1, B * N1, E)
    grads, jobs = [], []
    for j, (e, (h, w)) in enumerate(zip((e4, e3, e2), (hw[2], hw[1], hw[0]))):
        dz = _adjoint_to(dZ, B, H1, W1, h, w, E).view(1, B * h * w, E)
        sl = slice(slots[j] * E, (slots[j] + 1) * E)
        g = torch.empty_like(dz)
        jobs.append(dict(A=dz, B=Wf[:, :, sl].transpose(1, 2), C=g))
        grads.append(g.view(e.shape))
        _wgrad_into(dz, e.reshape(1, B * h * w, E), Wfg[:, :, sl])
    e1f = e1.reshape(1, B * N1, E)
    de1 = torch.empty_like(e1f)
    s1 = slice(slots[3] * E, (slots[3] + 1) * E)
    jobs.append(dict(A=dZ, B=Wf[:, :, s1].transpose(1, 2), C=de1))
    _wgrad_into(dZ, e1f, Wfg[:, :, s1], bfg)
    _gemm_group(jobs)                         # the four branches' input gradients: one launch
    return grads[0], grads[1], grads[2], de1.view(e1.shape), None, None, None, None, None, None


# CMX_DECODER_FOLD=0: linear_c{1..4} as their own GEMMs ahead of DecoderFuseF (A/B switch)
DECODER_FOLD = os.environ.get("CMX_DECODER_FOLD", "1") != "0"
# CMX_DECODER_UP3=1: DecoderFoldF's forward sums the three upsampled branches in a separate pass
# (cmx_bilinear_up3_add) and runs the c1 GEMM with it as a plain residual, instead of adding them
# in the c1 GEMM's epilogue (cmx_decoder_fuse_fwd).  Off: 38 + 27 us in the step against 57 for the
# epilogue form (round 6).  CMX_DECODER_ADJ3=0: the backward takes the three bilinear adjoints one
# grid at a time (2 launches each, dZ read three times) instead of from one read of dZ
# (cmx_bilinear_adjoint3: 55 against 79 us in the step)
DECODER_UP3 = os.environ.get("CMX_DECODER_UP3", "0") == "1"
DECODER_ADJ3 = os.environ.get("CMX_DECODER_ADJ3", "1") != "0"


def _up3_ok(E, ws):
    """cmx_bilinear_up3_add takes this decoder's shapes (its staging budget)."""
    return DECODER_UP3 and E % 64 == 0 and sum(ws) <= 160


def _adj3_ok(E, W1, ws, dtype):
    """cmx_bilinear_adjoint3 takes this decoder's shapes (its LDS budget)."""
    cs, esz = (64, 4) if dtype == torch.float32 else (128, 2)
    if not DECODER_ADJ3 or E % cs:
        return False
    taps = sum(w * ((2 * W1 + w - 1) // w + 3) for w in ws)
    return (2 * taps + 3) // 4 * 16 + W1 * cs * esz <= 65536


class DecoderFoldF(Function):
    """DecoderHead's four MLP projections, upsample, concat and linear_fuse 1x1 conv
    (MLPDecoder.py:60-77) with linear_c{1..4} folded into the conv.  Branch i of the reference
    is Wf_i up_i(x_i Wc_i^T + bc_i) (Wf_i: the conv's column slot of the branch, up_1 = identity);
    bilinear upsampling is linear with weights summing to 1, so

        Z = sum_i up_i(x_i M_i^T) + b,    M_i = Wf_i Wc_i  (E x C_i),    b = bf + sum_i Wf_i bc_i

    Forward: the four compositions M_i as one multi GEMM (K = E), b (cmx_decoder_fold_bias), the
    c2..c4 products x_i M_i^T at their own resolution (one multi launch) and the c1 product
    (K = C1 = 64 instead of the reference's two GEMMs with K = 64 and K = 512) with their
    bilinear upsample added in its epilogue (cmx_decoder_fuse_fwd).  Neither the (B, N1, 4E)
    concat nor the four (B, N_i, E) projections exist.  Backward, with dY_i = up_i^T dZ (the three
    bilinear adjoints from one read of dZ, cmx_bilinear_adjoint3):
    dx_i = dY_i M_i (one multi launch); dM_i = dY_i^T x_i and gb = sum_rows dZ are queued
    weight-gradient problems; after the flush that forms them (deferred.after) the chain rule

        dWf_i = dM_i Wc_i^T + gb bc_i^T    dWc_i = Wf_i^T dM_i    dbc_i = Wf_i^T gb    dbf = gb

    is one prep kernel (cmx_decoder_fold_bwd_prep: the 16-bit copy of dM, Wf^T, the rank-1 and
    bias terms) and two multi GEMMs of 512 x 512-sized products.  Executed per B2 step (bs=2):
    about 11 GFLOP forward + backward instead of 75 for DecoderFuseF on top of linear_c{1..4};
    the step roofline keeps the reference's op-by-op count (flops.py)."""

    # Wf column slot of the branches (c4, c3, c2, c1); Wc, bc and the gradient views come in slot order
    SLOTS = (0, 1, 2, 3)

    @staticmethod
    def forward(ctx, x4, x3, x2, x1, Wf, Wc, bf, bc, grads, sizes, anchor):
        return _decoder_fold_fwd(ctx, DecoderFoldF.SLOTS, x4, x3, x2, x1, Wf, Wc, bf, bc, grads, sizes)

    @staticmethod
    def backward(ctx, dZ):
        return _decoder_fold_bwd(ctx, dZ)


class DecoderFoldC1F(DecoderFoldF):
    """DecoderFoldF for a head whose concat is [c1 | c2 | c3 | c4] (MLPDecoderpp.py:80) and whose
    projections are 1x1 convs (:42-45, the same products): the same launches, branch j of
    (c4, c3, c2, c1) on column slot 3 - j of the conv; Wc, bc and the gradient views in slot order
    (c1 first)."""
    SLOTS = (3, 2, 1, 0)

    @staticmethod
    def forward(ctx, x4, x3, x2, x1, Wf, Wc, bf, bc, grads, sizes, anchor):
        return _decoder_fold_fwd(ctx, DecoderFoldC1F.SLOTS, x4, x3, x2, x1, Wf, Wc, bf, bc, grads, sizes)


def _decoder_fold_fwd(ctx, slots, x4, x3, x2, x1, Wf, Wc, bf, bc, grads, sizes):
    B, N1, C1 = x1.shape
    E = Wf.shape[0]
    (H1, W1), hw = sizes[0], sizes[1:]        # hw: grids of c2, c3, c4
    xs = (x4, x3, x2, x1)                     # branch order; branch j reads column slot slots[j] of Wf
    Cs = [w.shape[1] for w in Wc]
    Ms = [torch.empty(1, E, C, dtype=Wf.dtype, device=Wf.device) for C in Cs]
    _gemm_group([dict(A=Wf[None, :, s * E:(s + 1) * E], B=Wc[s][None].transpose(1, 2), C=Ms[s], splitk=1)
                 for s in range(4)])          # M_i = Wf_i Wc_i: one launch
    b = torch.empty(E, dtype=torch.float32, device=Wf.device)
    K.call("cmx_decoder_fold_bias", Wf, Wf.stride(0), bf, *bc, b, E, K.dtype_code(Wf))
    zs, jobs = [], []
    for j, (h, w) in enumerate((hw[2], hw[1], hw[0])):
        s = slots[j]
        z = torch.empty(1, B * h * w, E, dtype=x1.dtype, device=x1.device)
        jobs.append(dict(A=_c(xs[j]).reshape(1, B * h * w, Cs[s]), B=Ms[s], C=z))
        zs.append(z)
    _gemm_group(jobs)                         # the three low-resolution branch products: one launch
    if _up3_ok(E, [w for (_, w) in hw]):
        # b + the three upsampled products in one pass, then the c1 GEMM with it as the residual
        Z = torch.empty(B * N1, E, dtype=x1.dtype, device=x1.device)
        U = torch.empty(1, B * N1, E, dtype=x1.dtype, device=x1.device)
        K.call("cmx_bilinear_up3_add", zs[0], zs[1], zs[2], B, *hw[2], *hw[1], *hw[0], b, U, H1, W1, E,
               K.dtype_code(x1))
        K.gemm(_c(x1).view(1, B * N1, C1), Ms[slots[3]], Z.view(1, B * N1, E), residual=U)
    else:
        Z = K.decoder_fuse_fwd(_c(x1), Ms[slots[3]][0], b, zs, H1, W1, hw)
    ctx.save_for_backward(*xs, Wf, *Wc, *Ms)
    ctx.meta = (bc, grads, sizes, _adj3_ok(E, W1, [w for (_, w) in hw], x1.dtype), slots)
    return Z


def _decoder_fold_bwd(ctx, dZ):
    t = ctx.saved_tensors
    xs, Wf, Wc, Ms = t[:4], t[4], t[5:9], t[9:13]
    bc, grads, sizes, adj3, slots = ctx.meta
    B, N1, C1 = xs[3].shape
    E = Wf.shape[0]
    (H1, W1), hw = sizes[0], sizes[1:]
    Cs = [w.shape[1] for w in Wc]
    dZ = _c(dZ).view(1, B * N1, E)
    offs = [0]
    for C in Cs:
        offs.append(offs[-1] + E * C)
    dM = torch.empty(offs[-1], dtype=torch.float32, device=dZ.device)
    gb = torch.empty(1, E, dtype=torch.float32, device=dZ.device)
    if adj3:
        # the three grids' bilinear adjoints from one read of dZ (cmx_bilinear_adjoint3)
        dYs = [torch.empty(1, B * h * w, E, dtype=dZ.dtype, device=dZ.device) for (h, w) in (hw[2], hw[1], hw[0])]
        ts = [torch.empty(B * H1 * w * E, dtype=torch.float32, device=dZ.device) for (h, w) in (hw[2], hw[1], hw[0])]
        K.call("cmx_bilinear_adjoint3", dZ, *ts, *dYs, B, H1, W1, *hw[2], *hw[1], *hw[0], E, K.dtype_code(dZ))
    dxs, jobs = [], []
    for j in range(4):
        s = slots[j]
        if j == 3:
            dY = dZ
        elif adj3:
            dY = dYs[j]
        else:
            dY = _adjoint_to(dZ, B, H1, W1, *hw[2 - j], E).view(1, -1, E)
        x = xs[j].reshape(1, -1, Cs[s])
        dx = torch.empty_like(x)
        jobs.append(dict(A=dY, B=Ms[s].transpose(1, 2), C=dx))
        dxs.append(dx.view(xs[j].shape))
        _wgrad_into(dY, x, dM[offs[s]:offs[s + 1]].view(1, E, Cs[s]), gb if j == 3 else None)
    _gemm_group(jobs)                         # the four branches' input gradients: one launch
    deferred.after(lambda: _decoder_fold_chain(dM, gb, offs, Wf, Wc, bc, grads, Cs, E))
    return (*dxs, None, None, None, None, None, None, None)


def _decoder_fold_chain(dM, gb, offs, Wf, Wc, bc, grads, Cs, E):
    """DecoderFoldF's weight and bias gradients from dM_i (fp32, packed) and gb once they exist."""
    Wfg, bfg, Wcg, bcg = grads
    h16 = Wf.dtype != torch.float32
    dMh = torch.empty(dM.shape, dtype=Wf.dtype, device=dM.device) if h16 else None
    WfT = torch.empty(4 * E, E, dtype=Wf.dtype, device=Wf.device)
    K.call("cmx_decoder_fold_bwd_prep", dM, dMh, dM.numel(), gb, Wf, Wf.stride(0), WfT, Wfg, Wfg.stride(-2), *bc, *bcg,
           bfg, E, K.dtype_code(Wf))
    src = dMh if h16 else dM
    D = [src[offs[s]:offs[s + 1]].view(1, E, Cs[s]) for s in range(4)]
    # dWf_i += dM_i Wc_i^T (onto gb bc_i^T) and dWc_i = Wf_i^T dM_i: one launch each
    _gemm_group([dict(A=D[s], B=Wc[s][None], C=Wfg[:, :, s * E:(s + 1) * E], out_mode=2, splitk=1) for s in range(4)])
    _gemm_group([dict(A=WfT[None, s * E:(s + 1) * E], B=D[s].transpose(1, 2), C=Wcg[s], out_mode=1, splitk=1)
                 for s in range(4)])


# ---------------------------------------------------------------------------- final upsample + CE
def _scale_adjoint(ctx, adj, dloss, out):
    """The backward of the forward-adjoint losses: dlogits = adj * dloss / normaliser (out[1])."""
    dl = torch.empty(ctx.lshape, dtype=ctx.ldtype, device=adj.device)
    K.call("cmx_upsample_ce_bwd_scale", adj, dloss, out, dl, dl.numel(), K.dtype_code(dl))
    return dl


class UpsampleCEF(Function):
    """F.interpolate(logits, (H, W), bilinear) + CrossEntropyLoss(mean, ignore_index)
    (builder.py:233,249) fused; full-res logits are never materialised."""

    @staticmethod
    def forward(ctx, logits, label, dims, ignore):
        B, h, w, H, W, Kc = dims
        # exact x4 (every CMX config), K <= 40: with a backward to come, the loss and the bilinear
        # adjoint of (softmax - onehot) in one pass (cmx_upsample_ce_fwd_adj; the backward scales
        # it by dloss / n_valid); without one, the loss only.  Else the materialised-gradient path
        fused = H == 4 * h and W == 4 * w and Kc <= 40
        logits = _c(logits)
        grad = None if fused else torch.empty(B, H, W, Kc, dtype=logits.dtype, device=logits.device)
        out = torch.empty(3, dtype=torch.float32, device=logits.device)
        ws = K._ws(K.query("cmx_upsample_ce_workspace", B, H, W), logits.device)
        if fused and ctx.needs_input_grad[0]:
            adj = torch.empty(B, h * w, Kc, dtype=torch.float32, device=logits.device)
            K.call("cmx_upsample_ce_fwd_adj", logits, label, adj, out, ws, B, h, w, H, W, Kc, ignore,
                   K.dtype_code(logits))
            ctx.save_for_backward(adj, out, label)
            ctx.fused, ctx.ldtype, ctx.lshape = "adj", logits.dtype, logits.shape
            return out[0]
        K.call("cmx_upsample_ce_fwd", logits, label, grad, out, ws, B, h, w, H, W, Kc, ignore, K.dtype_code(logits))
        ctx.save_for_backward(logits if fused else grad, out, label)
        ctx.fused = fused
        ctx.dims = dims
        ctx.ldtype = logits.dtype
        ctx.lshape = logits.shape
        return out[0]             # a view of the kernel's result (no copy launch)

    @staticmethod
    def backward(ctx, dloss):
        grad, out, label = ctx.saved_tensors
        dloss = _c(dloss.reshape(1).to(torch.float32))
        if ctx.fused == "adj":
            return _scale_adjoint(ctx, grad, dloss, out), None, None, None
        # the materialised gradient (a fused loss-only forward ran without needs_input_grad:
        # autograd never comes here for it)
        B, h, w, H, W, Kc = ctx.dims
        tmp = torch.empty(B * H, w, Kc, dtype=torch.float32, device=grad.device)
        K.bilinear_adjoint_1d(grad, tmp, B * H, W, w, Kc, W * Kc, Kc)
        dl = torch.empty(B, h * w, Kc, dtype=ctx.ldtype, device=grad.device)
        K.bilinear_adjoint_1d(tmp, dl, B, H, h, w * Kc, H * w * Kc, w * Kc, a1=dloss, a2=out[1:])
        return dl.view(ctx.lshape), None, None, None


LOSS_WCE, LOSS_FOCAL2D, LOSS_FOCAL = 0, 1, 2     # cmx_upsample_loss_fwd_adj's `kind`


class UpsampleLossF(Function):
    """F.interpolate(logits, (H, W), bilinear) + one of the criteria beside plain CrossEntropyLoss
    (train.py:70-88) fused as UpsampleCEF's training form: the forward gives the loss and the unscaled
    fp32 bilinear adjoint of the per-pixel gradient in one pass (cmx_upsample_loss_fwd_adj), the backward
    scales it by dloss / normaliser (cmx_upsample_ce_bwd_scale).  spec = (kind, gamma, alpha, ce_scale,
    focal_scale); weight: K fp32 class weights on the logits' device, or None.  There is no
    materialised fallback: outside H = 4h, W = 4w, K <= 40 this raises NotImplementedError.  Without a
    backward to come (validation under no_grad) the same kernel runs and the adjoint is dropped."""

    @staticmethod
    def forward(ctx, logits, label, dims, ignore, spec, weight):
        B, h, w, H, W, Kc = dims
        kind, gamma, alpha, ce_scale, focal_scale = spec
        logits = _c(logits)
        if weight is not None and (weight.device != logits.device or weight.dtype != torch.float32
                                   or weight.numel() != Kc or not weight.is_contiguous()):
            raise ValueError(f"class weight: {Kc} contiguous fp32 values on {logits.device} expected")
        out = torch.empty(3, dtype=torch.float32, device=logits.device)
        adj = torch.empty(B, h * w, Kc, dtype=torch.float32, device=logits.device)
        ws = K._ws(K.query("cmx_upsample_loss_workspace", B, h, w), logits.device)
        if K.refusable("cmx_upsample_loss_fwd_adj", (K.CMX_ERR_SHAPE,), logits, label, weight, adj, out, ws, B, h, w, H,
                       W, Kc, ignore, int(kind), float(gamma), float(alpha), float(ce_scale), float(focal_scale),
                       K.dtype_code(logits)) is K.REFUSED:
            raise NotImplementedError(f"fused upsample + loss: {K.last_error()}; only CrossEntropyLoss has a "
                                      "materialised path for other shapes")
        ctx.save_for_backward(adj, out)
        ctx.ldtype, ctx.lshape = logits.dtype, logits.shape
        return out[0]             # a view of the kernel's result (no copy launch)

    @staticmethod
    def backward(ctx, dloss):
        adj, out = ctx.saved_tensors
        dloss = _c(dloss.reshape(1).to(torch.float32))
        return _scale_adjoint(ctx, adj, dloss, out), None, None, None, None, None


class UpsampleDiceF(Function):
    """F.interpolate(logits, (H, W), bilinear) + dice_scale * DiceLoss(smooth) + ce_scale *
    CrossEntropyLoss (utils/loss_opr.py: DiceLoss is (0, 1), DiceCELoss(alpha) is (1 - alpha, alpha))
    fused (cmx_upsample_dice_fwd_adj): a statistics pass and its finalize give the loss, then the
    gradient pass writes the fp32 bilinear adjoint, final up to dloss; the backward scales it
    (cmx_upsample_ce_bwd_scale).  spec = (ce_scale, dice_scale, smooth).  Without a backward to come the
    gradient pass is not launched.  No materialised fallback: outside H = 4h, W = 4w, K <= 40 this
    raises NotImplementedError."""

    @staticmethod
    def forward(ctx, logits, label, dims, ignore, spec):
        B, h, w, H, W, Kc = dims
        ce_scale, dice_scale, smooth = spec
        logits = _c(logits)
        f32 = dict(dtype=torch.float32, device=logits.device)
        out = torch.empty(3, **f32)
        stats = torch.empty(B, Kc, 3, **f32)
        adj = torch.empty(B, h * w, Kc, **f32) if ctx.needs_input_grad[0] else None
        ws = K._ws(K.query("cmx_upsample_dice_workspace", B, h, w, Kc), logits.device)
        if K.refusable("cmx_upsample_dice_fwd_adj", (K.CMX_ERR_SHAPE,), logits, label, adj, out, stats, ws, B, h, w, H,
                       W, Kc, ignore, float(ce_scale), float(dice_scale), float(smooth),
                       K.dtype_code(logits)) is K.REFUSED:
            raise NotImplementedError(f"fused upsample + Dice loss: {K.last_error()}; only CrossEntropyLoss has "
                                      "a materialised path for other shapes")
        ctx.save_for_backward(adj, out)
        ctx.ldtype, ctx.lshape = logits.dtype, logits.shape
        return out[0]             # a view of the kernel's result (no copy launch)

    @staticmethod
    def backward(ctx, dloss):
        adj, out = ctx.saved_tensors
        dloss = _c(dloss.reshape(1).to(torch.float32))
        return _scale_adjoint(ctx, adj, dloss, out), None, None, None, None


class UpsampleOhemF(Function):
    """F.interpolate(logits, (H, W), bilinear) + ProbOhemCrossEntropy2d(thresh, min_kept)
    (utils/loss_opr.py) fused (cmx_upsample_ohem_fwd_adj): a statistics pass writes every pixel's
    target-class probability, a device radix select finds threshold = max(thresh, min_kept-th smallest),
    and the gradient pass is plain CE over the pixels at or below it; the backward scales the fp32
    bilinear adjoint by dloss / n_kept (cmx_upsample_ce_bwd_scale).  spec = (thresh, min_kept).  Nothing is
    read back to the host: the regime is chosen on the device.  Without a backward to come the same
    launches run and the adjoint is dropped.  No materialised fallback: outside H = 4h, W = 4w, K <= 40
    this raises NotImplementedError.  ``last`` = (out, counts) of the latest forward: out =
    [loss, 1 / n_kept, n_kept, threshold], counts = [n_valid, n_below, n_kept]."""

    last = None

    @staticmethod
    def forward(ctx, logits, label, dims, ignore, spec):
        B, h, w, H, W, Kc = dims
        thresh, min_kept = spec
        logits = _c(logits)
        f32 = dict(dtype=torch.float32, device=logits.device)
        out = torch.empty(4, **f32)
        py = torch.empty(B, H, W, **f32)
        counts = torch.empty(3, dtype=torch.int64, device=logits.device)
        adj = torch.empty(B, h * w, Kc, **f32)
        ws = K._ws(K.query("cmx_upsample_ohem_workspace", B, h, w), logits.device)
        if K.refusable("cmx_upsample_ohem_fwd_adj", (K.CMX_ERR_SHAPE,), logits, label, adj, out, py, counts, ws, B, h, w,
                       H, W, Kc, ignore, float(thresh), int(min_kept), K.dtype_code(logits)) is K.REFUSED:
            raise NotImplementedError(f"fused upsample + OHEM loss: {K.last_error()}; only CrossEntropyLoss has "
                                      "a materialised path for other shapes")
        UpsampleOhemF.last = (out, counts)
        ctx.save_for_backward(adj, out)
        ctx.ldtype, ctx.lshape = logits.dtype, logits.shape
        return out[0]             # a view of the kernel's result (no copy launch)

    @staticmethod
    def backward(ctx, dloss):
        adj, out = ctx.saved_tensors
        dloss = _c(dloss.reshape(1).to(torch.float32))
        return _scale_adjoint(ctx, adj, dloss, out), None, None, None, None


LOSS_CE = -1     # cmx_upsample_loss_scaled_fwd_adj's `kind` for plain CrossEntropyLoss
LOSS_SCALES = (8, 16, 32)


class UpsampleScaledLossF(Function):
    """F.interpolate(logits, scale_factor=S, bilinear) + a per-pixel criterion at the scales of an FCN head
    (S in 8, 16, 32: the stage-3 auxiliary head is x16, the FCN-32s decode head x32) fused as UpsampleLossF
    is at x4 (cmx_upsample_loss_scaled_fwd_adj, include/cmx_fcn.h): one pass over the labels gives the loss
    and the unscaled fp32 bilinear adjoint of the per-pixel gradient; the backward scales it by dloss /
    normaliser (cmx_upsample_ce_bwd_scale).  spec None: plain CrossEntropyLoss; otherwise UpsampleLossF's
    (kind, gamma, alpha, ce_scale, focal_scale).  weight as UpsampleLossF's.  S comes from dims: an (H, W)
    that is not exactly (S h, S w) with S in the set raises NotImplementedError.  Without a backward to come
    the same kernel runs and the adjoint is dropped."""

    @staticmethod
    def forward(ctx, logits, label, dims, ignore, spec, weight):
        B, h, w, H, W, Kc = dims
        S = H // h if h > 0 else 0
        if S not in LOSS_SCALES or H != S * h or W != S * w:
            raise NotImplementedError(f"fused upsample + loss at the scale of an FCN head: {h}x{w} -> {H}x{W} is not "
                                      f"an exact scale in {LOSS_SCALES}")
        kind, gamma, alpha, ce_scale, focal_scale = (LOSS_CE, 0.0, 0.0, 1.0, 0.0) if spec is None else spec
        logits = _c(logits)
        if weight is not None and (weight.device != logits.device or weight.dtype != torch.float32
                                   or weight.numel() != Kc or not weight.is_contiguous()):
            raise ValueError(f"class weight: {Kc} contiguous fp32 values on {logits.device} expected")
        out = torch.empty(3, dtype=torch.float32, device=logits.device)
        adj = torch.empty(B, h * w, Kc, dtype=torch.float32, device=logits.device)
        ws = K._ws(K.query("cmx_upsample_loss_scaled_workspace", B, h, w, S), logits.device)
        if K.refusable("cmx_upsample_loss_scaled_fwd_adj", (K.CMX_ERR_SHAPE,), logits, label, weight, adj, out, ws, B,
                       h, w, S, Kc, ignore, int(kind), float(gamma), float(alpha), float(ce_scale), float(focal_scale),
                       K.dtype_code(logits)) is K.REFUSED:
            raise NotImplementedError(f"fused upsample + loss at the scale of an FCN head: {K.last_error()}")
        if not ctx.needs_input_grad[0]:
            return out[0]
        ctx.save_for_backward(adj, out)
        ctx.ldtype, ctx.lshape = logits.dtype, logits.shape
        return out[0]             # a view of the kernel's result (no copy launch)

    @staticmethod
    def backward(ctx, dloss):
        adj, out = ctx.saved_tensors
        dloss = _c(dloss.reshape(1).to(torch.float32))
        return _scale_adjoint(ctx, adj, dloss, out), None, None, None, None, None


def upsample_logits_nchw(logits, B, h, w, H, W, Kc):
    out = torch.empty(B, Kc, H, W, dtype=torch.float32, device=logits.device)
    K.call("cmx_bilinear_fwd_nchw_f32", _c(logits), out, B, h, w, H, W, Kc, K.dtype_code(logits))
    return out
