"""Tensor-level wrappers over the C-ABI, one per entry point (or short protocol) that the package
calls from two or more places; a single-use entry point is called through ``call`` in the header's
argument order (_lib: a tensor, None or an integer address per pointer; the trailing stream is filled).

Every function launches on torch's current stream, allocates outputs/workspaces through
torch's caching allocator (so HIP-graph capture works) and raises CMXError on failure.
Activations are token-major and contiguous unless a stride argument says otherwise.
"""
from __future__ import annotations

import collections
import ctypes
import torch

from . import _lib
from ._lib import (call, try_call, query, refusable, last_error, ptr, stream, dtype_code,  # noqa: F401
                   REFUSED, CMX_ERR_ARG, CMX_ERR_SHAPE)

ACT = {"none": 0, "gelu": 1, "relu": 2, "sigmoid": 3}


def tune(name: str, value: int) -> None:
    """Set launch-policy knob `name` (e.g. "GEMM_SMALLK"; cmx_tune) for launches planned from now on."""
    call("cmx_tune", name.encode(), int(value))


def tune_get(name: str) -> int:
    """Current value of knob `name`, -1 if it has not been set or read yet."""
    return query("cmx_tune_get", name.encode())


def _ws(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(1, (nbytes + 3) // 4), dtype=torch.float32, device=device)


def tickets(cache: dict, entry: str, owner, x, B, C, least: int = 0) -> torch.Tensor:
    """Zeroed arrival counters (``entry``(B, C) of them, at least ``least``; each launch leaves them zero): one set in
    ``cache`` per (module -- ``owner`` is its anchor Parameter -- device, size), so launches that may run concurrently
    (two models, two streams) never share them.  Allocated at the first, eager call (before any HIP-graph capture)."""
    key = (id(owner), x.device, B, C)
    t = cache.get(key)
    if t is None:
        t = cache[key] = torch.zeros(max(least, query(entry, B, C)), dtype=torch.int32, device=x.device)
    return t


# ------------------------------------------------------------------------------ LayerNorm
def layernorm_fwd(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, G: int = 1,
                  save_stats: bool = True):
    """x (G*R, C) (any leading shape, contiguous); gamma/beta (G, C) fp32."""
    C = x.shape[-1]
    rows = x.numel() // C
    R = rows // G
    y = torch.empty_like(x)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device) if save_stats else None
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device) if save_stats else None
    call("cmx_layernorm_fwd", x, gamma, beta, y, mean, rstd, R, G, C, float(eps), dtype_code(x))
    return y, mean, rstd


def _ln_bwd_buffers(x, G):
    """(R, C, dx, workspace, the workspace seen as (G, nb, 2C) = [dgamma | dbeta] partials per block)."""
    C = x.shape[-1]
    R = x.numel() // C // G
    nbytes = query("cmx_layernorm_bwd_workspace", R, G, C, dtype_code(x))
    ws = _ws(nbytes, x.device)
    nb = nbytes // (8 * G * C)
    return R, C, torch.empty_like(x), ws, ws[:G * nb * 2 * C].view(G, nb, 2 * C)


def layernorm_bwd(dy, x, gamma, mean, rstd, G: int, dgamma: torch.Tensor | None, dbeta: torch.Tensor | None,
                  accumulate: bool = False):
    """Returns dx; with dgamma = dbeta = None (the deferred mode) (dx, partials) as layernorm_bwd_res does."""
    R, C, dx, ws, part = _ln_bwd_buffers(x, G)
    call("cmx_layernorm_bwd", dy, x, gamma, mean, rstd, dx, dgamma, dbeta, ws, R, G, C, accumulate, dtype_code(x))
    return dx if dgamma is not None or dbeta is not None else (dx, part)


def layernorm_bwd_res(dy, x, gamma, mean, rstd, G: int, dgamma=None, dbeta=None, dy2=None, dres=None, sscale=None,
                      rows_per_sample: int = 1, dxs=None, accumulate: bool = False):
    """cmx_layernorm_bwd_res: upstream dy + dy2, dx = dres + LN_bwd, dxs = sscale[row // rows_per_sample] * dx
    (dy2 / dres / sscale / dxs optional; dxs is the caller's).  Returns (dx, partials): with dgamma = dbeta =
    None nothing is reduced and partials, the workspace seen as (G, nb, 2C) = [dgamma | dbeta] per block,
    is what the caller reduces (the deferred mode)."""
    R, C, dx, ws, part = _ln_bwd_buffers(x, G)
    call("cmx_layernorm_bwd_res", dy, dy2, x, gamma, mean, rstd, dres, sscale, dxs, dx, dgamma, dbeta, ws, R, G, C,
         int(rows_per_sample), accumulate, dtype_code(x))
    return dx, part


# ------------------------------------------------------------------------------ elementwise
def residual_add(x, y, sample_scale=None, out=None, n_per_sample=None):
    out = torch.empty_like(x) if out is None else out
    nps = n_per_sample if n_per_sample is not None else x.numel()
    call("cmx_residual_add", x, y, sample_scale, out, nps, x.numel(), dtype_code(x))
    return out


def scale_samples(x, sample_scale, n_per_sample, out=None):
    out = torch.empty_like(x) if out is None else out
    call("cmx_scale_samples", x, sample_scale, out, n_per_sample, x.numel(), dtype_code(x))
    return out


def act_fwd(x, act: str, out=None):
    out = torch.empty_like(x) if out is None else out
    call("cmx_act_fwd", x, out, x.numel(), ACT[act], dtype_code(x))
    return out


def act_bwd(dy, z, act: str, out=None):
    out = torch.empty_like(dy) if out is None else out
    call("cmx_act_bwd", dy, z, out, dy.numel(), ACT[act], dtype_code(dy))
    return out


def cast_f32_bf16(src: torch.Tensor, dst: torch.Tensor):
    assert src.dtype == torch.float32 and dst.dtype == torch.bfloat16 and src.numel() == dst.numel()
    call("cmx_cast_f32_bf16", src, dst, src.numel())


def cast_f32_h16(src: torch.Tensor, dst: torch.Tensor):
    """fp32 -> bf16 / fp16 (round to nearest even) into ``dst``'s dtype."""
    assert src.dtype == torch.float32 and dst.dtype in (torch.bfloat16, torch.float16) and src.numel() == dst.numel()
    call("cmx_cast_f32_h16", src, dst, src.numel(), dtype_code(dst))
    return dst


def colsum(x: torch.Tensor, out: torch.Tensor, G: int = 1, accumulate: bool = False, alpha: float = 1.0,
           ld: int | None = None, N: int | None = None):
    """out (G, N) fp32 (+)= alpha * sum over rows of x viewed as (G, M, ld)[:, :, :N]."""
    ld = ld if ld is not None else x.shape[-1]
    N = N if N is not None else x.shape[-1]
    M = x.shape[:-1].numel() // G
    ws = _ws(query("cmx_colsum_workspace", M, G, N), x.device)
    call("cmx_colsum", x, out, ws, M, G, N, ld, accumulate, float(alpha), dtype_code(x))
    return out


def partials_sum(part: torch.Tensor, out: torch.Tensor, G: int, nblk: int, W: int, accumulate: bool = False):
    """out (G, W) fp32 (+)= the sum of the nblk partial rows of part (G, nblk, W) (cmx_partials_sum)."""
    call("cmx_partials_sum", part, out, G, nblk, W, accumulate, 1.0)
    return out


# ------------------------------------------------------------------------------ tiny-M linear (fp32 GEMV chains)
def small_linear_fwd(x: torch.Tensor, W, b, Nout: int, act: str = "none") -> torch.Tensor:
    """y (M, Nout) fp32 = act(x W^T + b) on x (M, K) fp32, M <= 8 (cmx_small_linear_fwd)."""
    M, Kin = x.shape
    y = torch.empty(M, Nout, dtype=torch.float32, device=x.device)
    call("cmx_small_linear_fwd", x, W, b, y, M, Kin, Nout, ACT[act])
    return y


def small_linear_bwd(dy_part, nslice: int, slice_stride: int, row_stride: int, y, x, W, dW, db, Nout: int,
                     act: str = "none") -> torch.Tensor:
    """small_linear_fwd's backward (cmx_small_linear_bwd): dy[m][n] = sum_s dy_part[s * slice_stride + m * row_stride
    + n] over nslice slabs; writes dW / db, returns dx as cmx_small_linear_nslice() partial slices (ns, M, K)."""
    M, Kin = x.shape
    dx_part = torch.empty(query("cmx_small_linear_nslice"), M, Kin, dtype=torch.float32, device=x.device)
    call("cmx_small_linear_bwd", dy_part, nslice, slice_stride, row_stride, y, x, W, dx_part, dW, db, M, Kin, Nout,
         ACT[act], 0)
    return dx_part


# ------------------------------------------------------------------------------ GEMM
def _operand(t: torch.Tensor, name: str | None = None):
    """(G, rows, k) logical view -> (trans, ld, batch stride); with neither stride a unit one: None, or the
    ValueError of a caller that names the operand."""
    if t.stride(2) == 1:
        return 0, t.stride(1), t.stride(0)
    if t.stride(1) == 1:
        return 1, t.stride(2), t.stride(0)
    if name is not None:
        raise ValueError(f"gemm: operand {name} needs a unit stride along rows or k, got strides {t.stride()}")
    return None


def gemm(A: torch.Tensor, B: torch.Tensor, C: torch.Tensor, bias: torch.Tensor | None = None,
         residual: torch.Tensor | None = None, rscale: torch.Tensor | None = None, rows_per_sample: int = 1,
         act: str = "none", out_mode: int = 0, A2: torch.Tensor | None = None, dbias: torch.Tensor | None = None,
         splitk: int = 0, plan: bool = False, mask: torch.Tensor | None = None):
    """C[g] = epi([A[g] | A2[g]] @ B[g]^T) on logical views A (G, M, K1), A2 (G, M, K-K1),
    B (G, N, K), C (G, M, N).

    A transposed operand is just a transposed view (unit stride along rows instead of k):
    the kernel reads it in place.  out_mode: 0 store in C's dtype (= A's), 1 store fp32,
    2 accumulate into fp32 C.  bias (G, N) fp32 (any batch stride, unit inner stride);
    residual has C's layout: C = residual + rscale[(g*M + i) // rows_per_sample] * act(acc + bias).
    dbias (G, M) fp32: also produce sum_k A(i, k) (the bias gradient of a wgrad).
    splitk > 1 splits K over blocks into fp32 slabs reduced with the epilogue applied;
    0 = the library's choice (cmx_gemm_splitk: fill the chip when the output has few tiles).
    mask (C's layout and dtype): C = 0 where mask <= 0, after the residual (a ReLU backward).
    plan=True: nothing is launched; returns a GemmPlan for gemm_multi, or None when the problem
    is not eligible for a multi launch (the caller then runs gemm as usual)."""
    G, M, K1 = A.shape
    Kd = K1 + (A2.shape[2] if A2 is not None else 0)
    N = B.shape[1]
    assert B.shape == (G, N, Kd) and C.shape == (G, M, N) and C.stride(2) == 1, (A.shape, B.shape, C.shape)
    assert A.dtype == B.dtype and C.dtype == (A.dtype if out_mode == 0 else torch.float32), (A.dtype, C.dtype)
    tA, lda, sA = _operand(A, "A")
    tA2, lda2, sA2 = _operand(A2, "A2") if A2 is not None else (0, 0, 0)
    assert tA2 == 0 and (A2 is None or (tA == 0 and A2.shape[:2] == (G, M) and A2.dtype == A.dtype))
    tB, ldb, sB = _operand(B, "B")
    sbias = 0
    if bias is not None:
        assert bias.dtype == torch.float32 and bias.shape[-1] == N and bias.stride(-1) == 1
        sbias = bias.stride(0) if bias.dim() == 2 else 0
    sdb = 0
    if dbias is not None:
        assert dbias.dtype == torch.float32 and dbias.shape[-1] == M and dbias.stride(-1) == 1
        sdb = dbias.stride(0) if dbias.dim() == 2 else 0
    if residual is not None:
        assert residual.shape == C.shape and residual.stride() == C.stride() and residual.dtype == C.dtype
    if mask is not None:
        assert mask.shape == C.shape and mask.stride() == C.stride() and mask.dtype == C.dtype and out_mode == 0
    Nk = N + (1 if dbias is not None else 0)
    if splitk <= 0:
        splitk = query("cmx_gemm_splitk", G, M, Nk, Kd, dbias is not None, dtype_code(A))
    args = (G, M, Nk, Kd, K1, lda, lda2, ldb, C.stride(1), sA, sA2, sB, C.stride(0), sbias, sdb, int(rows_per_sample),
            tA, tB, ACT[act], int(out_mode), dbias is not None, int(splitk), dtype_code(A))
    if plan:
        if splitk > 1:
            return None
        rec = (ctypes.c_uint8 * _PLAN_BYTES)()
        nb = query("cmx_gemm_plan", ctypes.addressof(rec), A, A2, B, C, bias, residual, rscale, mask, dbias, None,
                   *args)
        if nb < 0:
            raise _lib.CMXError(f"cmx_gemm_plan failed ({nb}): {_lib.last_error()}")
        return GemmPlan(rec, (A, A2, B, C, bias, residual, rscale, mask)) if nb > 0 else None
    ws = _ws(query("cmx_gemm_workspace", G, M, Nk, splitk), A.device) if splitk > 1 else None
    call("cmx_gemm", A, A2, B, C, bias, residual, rscale, mask, dbias, ws, *args)
    return C


def gemm_ln(A, B, C, ln_gamma, ln_beta, ln_eps, bias=None, residual=None, rscale=None, rows_per_sample=1,
            act="none", A2=None):
    """K.gemm's forward form (C = epi(A @ B^T)) plus the LayerNorm of C's rows in the same
    launch (cmx_gemm_ln): returns (y, mean, rstd), y = LN(C) in C's layout, mean / rstd (G, M)
    fp32; None when the problem is not eligible (the caller runs gemm + the LN kernel).
    N <= 128 (N % 8 == 0): the LayerNorm runs in the GEMM's epilogue (one tile spans a row)."""
    G, M, K1 = A.shape
    Kd = K1 + (A2.shape[2] if A2 is not None else 0)
    N = B.shape[1]
    if A.dtype not in (torch.bfloat16, torch.float16) or not (N <= 128 and N % 8 == 0) or not C.is_contiguous():
        return None
    tA, lda, sA = _operand(A, "A")
    tB, ldb, sB = _operand(B, "B")
    _, lda2, sA2 = _operand(A2, "A2") if A2 is not None else (0, 0, 0)
    if tA or tB:
        return None
    sbias = (bias.stride(0) if bias.dim() == 2 else 0) if bias is not None else 0
    y = torch.empty_like(C)
    mean = torch.empty(G, M, dtype=torch.float32, device=C.device)
    rstd = torch.empty_like(mean)
    if refusable("cmx_gemm_ln", (CMX_ERR_ARG,), A, A2, B, C, bias, residual, rscale, G, M, N, Kd, K1, lda, lda2, ldb,
                 C.stride(1), sA, sA2, sB, C.stride(0), sbias, int(rows_per_sample), ACT[act], ln_gamma, ln_beta,
                 ln_gamma.stride(0) if ln_gamma.dim() == 2 else 0, float(ln_eps), y, mean, rstd,
                 dtype_code(A)) is REFUSED:
        return None
    return y, mean, rstd


def gemm_ln_bwd(dz, W, x, gamma, mean, rstd, dres=None, dy2=None, sscale=None, rows_per_sample=1, dxs=None):
    """dx of the LayerNorm that produced a Linear's input, with the Linear's input gradient
    dy = dz @ W (dz (G, M, K), W (G, K, N) = the weight's (out, in) view) computed in the same launch
    (cmx_gemm_ln_bwd): dx = LN'(dy [+ dy2]) + dres; dxs (when given) = sscale[row // rps] * dx.
    Returns (dx, partials (G, ceil(M / 64), 2N) fp32: dgamma | dbeta per 64-row tile), or None when
    not eligible (the caller runs the dgrad GEMM and the LayerNorm backward kernel)."""
    G, M, Kd = dz.shape
    N = W.shape[2]
    if dz.dtype not in (torch.bfloat16, torch.float16) or N > 128 or N % 8 or not dz.is_contiguous() \
            or not x.is_contiguous() or W.shape[:2] != (G, Kd):
        return None
    tB, ldb, sB = _operand(W.transpose(1, 2), "B")
    if not tB:
        return None
    dx = torch.empty_like(x)
    part = torch.empty(G, (M + 63) // 64, 2 * N, dtype=torch.float32, device=x.device)
    if refusable("cmx_gemm_ln_bwd", (CMX_ERR_ARG,), dz, W, dx, G, M, N, Kd, dz.stride(1), ldb, x.stride(1),
                 dz.stride(0), sB, x.stride(0), x, gamma, gamma.stride(0) if gamma.dim() == 2 else 0, mean, rstd, dres,
                 dy2, sscale, int(rows_per_sample), dxs, part, dtype_code(dz)) is REFUSED:
        return None
    return dx, part


def conv_patch_dgrad_ln_bwd(dy, W, geom, x, gamma, mean, rstd, dres=None, dy2=None, sscale=None, rows_per_sample=1,
                            dxs=None):
    """dx of the LayerNorm that produced a non-overlapping patchify conv's input, with the conv's
    input gradient col2im(dy @ W) computed in the same launch (cmx_conv_patch_dgrad_ln_bwd).
    dy (G, NIg*Ho*Wo, N), W (G, N, R*R*C) tap-major, x / dres / dy2 / dxs NHWC (G*NIg, H, W, C).
    Returns (dx, partials (G, nb, 2C)) or None when not eligible."""
    G, NIg, H, Wd, C, R, Ho, Wo = geom
    if dy.dtype not in (torch.bfloat16, torch.float16) or C not in (64, 128) or Ho * R != H or Wo * R != Wd \
            or not (dy.is_contiguous() and x.is_contiguous()):
        return None
    dx = torch.empty_like(x)
    nb = (NIg * Ho * Wo + 63) // 64 * R * R
    part = torch.empty(G, nb, 2 * C, dtype=torch.float32, device=x.device)
    if refusable("cmx_conv_patch_dgrad_ln_bwd", (CMX_ERR_ARG, CMX_ERR_SHAPE), dy, W, dx, G, NIg, H, Wd, C, R, Ho, Wo,
                 W.shape[1], dy.stride(0), W.stride(0), NIg * H * Wd * C, x, gamma,
                 gamma.stride(0) if gamma.dim() == 2 else 0, mean, rstd, dres, dy2, sscale, int(rows_per_sample), dxs,
                 part, dtype_code(dy)) is REFUSED:
        return None
    return dx, part


def conv_patch_dgrad(dy, W, dx, geom):
    """dx (the caller's) = col2im(dy @ W) alone (cmx_conv_patch_dgrad); layouts, geom: conv_patch_dgrad_ln_bwd's."""
    G, NIg, H, Wd, C, R, Ho, Wo = geom
    call("cmx_conv_patch_dgrad", dy, W, dx, G, NIg, H, Wd, C, R, Ho, Wo, W.shape[1], dy.stride(0), W.stride(0),
         NIg * H * Wd * C, dtype_code(dy))
    return dx


_PLAN_BYTES = query("cmx_gemm_plan_size")


class GemmPlan:
    """A planned 64 x 64-tile GEMM (cmx_gemm_plan) and the tensors it reads / writes."""

    def __init__(self, rec, keep):
        self.rec, self.keep = rec, keep


def gemm_multi(plans) -> None:
    """Launch up to four planned GEMMs (same dtype and B layout) as ONE grid (cmx_gemm_multi)."""
    n = len(plans)
    buf = (ctypes.c_uint8 * (_PLAN_BYTES * n))()
    for i, p in enumerate(plans):
        ctypes.memmove(ctypes.addressof(buf) + i * _PLAN_BYTES, p.rec, _PLAN_BYTES)
    call("cmx_gemm_multi", ctypes.addressof(buf), n)


def gemm_h2(A: torch.Tensor, B: torch.Tensor, C: torch.Tensor, out_mode: int = 0, splitk: int = 0) -> torch.Tensor:
    """C[o, h] = A[o, h] @ B[o, h]^T over a two-level batch of logical 4-D views A (Go, gh, M, K),
    B (Go, gh, N, K), C (Go, gh, M, N) (cmx_gemm_h2): e.g. per-head products whose heads are
    column slices of token rows, so the (image, head) pairs have no single batch stride."""
    Go, gh, M, K = A.shape
    N = B.shape[2]
    assert B.shape == (Go, gh, N, K) and C.shape == (Go, gh, M, N) and C.stride(3) == 1, (A.shape, B.shape, C.shape)
    assert A.dtype == B.dtype and C.dtype == (A.dtype if out_mode == 0 else torch.float32), (A.dtype, C.dtype)

    def op(t, name):
        if t.stride(3) == 1:
            return 0, t.stride(2)
        if t.stride(2) == 1:
            return 1, t.stride(3)
        raise ValueError(f"gemm_h2: operand {name} needs a unit stride along rows or k, got {t.stride()}")
    tA, lda = op(A, "A")
    tB, ldb = op(B, "B")
    G = Go * gh
    if splitk <= 0:
        splitk = query("cmx_gemm_splitk", G, M, N, K, 0, dtype_code(A))
    ws = _ws(query("cmx_gemm_workspace", G, M, N, splitk), A.device) if splitk > 1 else None
    call("cmx_gemm_h2", A, B, C, ws, G, gh, M, N, K, lda, ldb, C.stride(2), A.stride(0), A.stride(1), B.stride(0),
         B.stride(1), C.stride(0), C.stride(1), tA, tB, int(out_mode), int(splitk), dtype_code(A))
    return C


# ------------------------------------------------------------------------------ SRA attention
SRA_PATHS = ("general", "fast", "small")
SraPlan = collections.namedtuple("SraPlan", "fwd bwd qw nw dkv_chunks dkv_direct dq_seq cus")


def sra_plan(Bt, N, Nk, heads, D, dtype, aligned=True) -> SraPlan:
    """The launch decision sra_attn_fwd / sra_attn_bwd take for this problem under the current knobs
    (cmx_sra_plan; nothing is launched).  fwd / bwd: "general", "fast" or "small"; (qw, nw): the
    instantiation of the fast forward / dQ (0 when neither is fast); dkv_chunks: query chunks of the
    dK / dV kernel; dkv_direct: it stores dK / dV itself (no fp32 slabs, no reduce launch); dq_seq: the
    short-sequence dQ form; cus: the CU count used.  aligned: every row on 16 B (False: none; an int is
    passed through, bit 0 = q, k, v, o, dO, dq and bit 1 = dK / dV)."""
    code = _lib.DTYPE_CODES[dtype]
    out = (ctypes.c_int32 * 8)()
    call("cmx_sra_plan", ctypes.addressof(out), 8, Bt, N, Nk, heads, D, code, 3 if aligned is True else int(aligned))
    f = list(out)
    return SraPlan(SRA_PATHS[f[0]], SRA_PATHS[f[1]], f[2], f[3], f[4], bool(f[5]), bool(f[6]), f[7])


def sra_attn_fwd(q, k, v, Bt, N, Nk, heads, D, scale, qs, kvs, save_lse=True):
    """q: base pointer tensor of (Bt, N, *) rows with stride qs; k/v: views into the kv
    projection (k = kv[..., :C], v = kv[..., C:]) with row stride kvs."""
    o = torch.empty(Bt, N, heads * D, dtype=q.dtype, device=q.device)
    lse = torch.empty(Bt, heads, N, dtype=torch.float32, device=q.device) if save_lse else None
    call("cmx_sra_attn_fwd", q, k, v, o, lse, Bt, N, Nk, heads, D, qs, kvs, heads * D, float(scale), dtype_code(q))
    return o, lse


def sra_attn_bwd(q, k, v, o, dout, lse, Bt, N, Nk, heads, D, scale, qs, kvs, dkv=None):
    """Returns (dq (Bt, N, heads*D), dkv (Bt, Nk, 2*heads*D))."""
    C = heads * D
    dq = torch.empty(Bt, N, C, dtype=q.dtype, device=q.device)
    if dkv is None:
        dkv = torch.empty(Bt, Nk, 2 * C, dtype=q.dtype, device=q.device)
    ws = _ws(query("cmx_sra_attn_bwd_workspace", Bt, N, Nk, heads, D), q.device)
    call("cmx_sra_attn_bwd", q, k, v, o, dout, lse, dq, dkv, dkv[..., C:], ws, Bt, N, Nk, heads, D, qs, kvs, C, C, C,
         2 * C, float(scale), dtype_code(q))
    return dq, dkv


# ------------------------------------------------------------------------------ conv (im2col, stage-1 direct)
def im2col_nhwc(x, cols, NI, H, Wd, C, KH, KW, st, pad, Ho, Wo):
    """cols (G, NI/G*Ho*Wo, Kp), the caller's, = the im2col columns of x NHWC (NI, H, Wd, C) (cmx_im2col_nhwc)."""
    call("cmx_im2col_nhwc", x, cols, NI, H, Wd, C, KH, KW, st, pad, Ho, Wo, cols.shape[-1], dtype_code(cols))
    return cols


def pe1_conv_fwd(img0, img1, W, b, geom, ln=None):
    """y (G, Bg*Ho*Wo, N), W's dtype = the stage-1 conv straight from the fp32 NCHW batches img0 / img1 (one launch,
    cmx_pe1_conv_fwd); geom = (G, Bg, C, H, Wd, KH, KW, stride, pad, Ho, Wo); ln = (gamma, beta, eps): also the
    LayerNorm of y's rows, in the same epilogue, and (y, LN(y), mean, rstd) is returned."""
    G, Bg, Ho, Wo = *geom[:2], *geom[-2:]
    y = torch.empty(G, Bg * Ho * Wo, W.shape[1], dtype=W.dtype, device=W.device)
    gamma, beta, eps = ln if ln is not None else (None, None, 0.0)
    out = torch.empty_like(y) if ln is not None else None
    mean = torch.empty(G * Bg * Ho * Wo, dtype=torch.float32, device=W.device) if ln is not None else None
    rstd = torch.empty_like(mean) if ln is not None else None
    call("cmx_pe1_conv_fwd", img0, img1, W, b, y, *geom, W.shape[1], W.shape[-1], W.stride(0), b.stride(0), y.stride(0),
         gamma, beta, out, mean, rstd, gamma.stride(0) if ln is not None else 0, float(eps), dtype_code(W))
    return y if ln is None else (y, out, mean, rstd)


def pe1_conv_wgrad(dy, img0, img1, geom, N, Kp):
    """The stage-1 conv's weight and bias gradient as per-workgroup partial slabs (G, nblk, N, Kp + 1) =
    [dW | db] fp32 for the caller to reduce (cmx_pe1_conv_wgrad); geom as pe1_conv_fwd's."""
    nblk = query("cmx_pe1_conv_wgrad_nblk", geom[1], *geom[-2:])
    ws = torch.empty(geom[0], nblk, N, Kp + 1, dtype=torch.float32, device=dy.device)
    call("cmx_pe1_conv_wgrad", dy, img0, img1, ws, *geom, N, Kp, dy.stride(0), dtype_code(dy))
    return ws


# ------------------------------------------------------------------------------ FRM pooling, BatchNorm scratch
def frm_pool_fwd(x, tk):
    """avg || max pooling of x (2, B, N, C) over N (cmx_frm_pool_fwd): pooled (B, 4C) fp32, argmax (B, 2C) int32;
    tk: the call site's arrival counters (functions.pool_tickets)."""
    _, B, N, C = x.shape
    pooled = torch.empty(B, 4 * C, dtype=torch.float32, device=x.device)
    argmax = torch.empty(B, 2 * C, dtype=torch.int32, device=x.device)
    ws = _ws(query("cmx_frm_pool_workspace", B, N, C), x.device)
    call("cmx_frm_pool_fwd", x, pooled, argmax, ws, tk, B, N, C, dtype_code(x))
    return pooled, argmax


def frm_pool_bwd(dpooled_part, argmax, dx):
    """dx (2, B, N, C) += the pooling backward of dpooled, given as small_linear_bwd's (nslice, B, 4C) slices."""
    _, B, N, C = dx.shape
    call("cmx_frm_pool_bwd", dpooled_part, dpooled_part.shape[0], B * 4 * C, argmax, dx, B, N, C, dtype_code(dx))


def bn_scratch(M, C, device):
    """(sums (2, C), workspace) fp64 of the BatchNorm statistics / backward-reduce kernels."""
    sums = torch.empty(2, C, dtype=torch.float64, device=device)
    return sums, torch.empty(max(1, query("cmx_bn_workspace", M, C) // 8), dtype=torch.float64, device=device)


# ------------------------------------------------------------------------------ decoder
def bilinear_adjoint_1d(src, out, P, Lo, Li, Q, sp, so, a1=None, a2=None):
    """One separable pass of the bilinear adjoint, Lo -> Li samples along one axis, into out (the caller's), in the
    tensors' dtypes (cmx_bilinear_adjoint_1d); a1 / a2 (1-element fp32, optional): scaled by a1[0] / a2[0]."""
    call("cmx_bilinear_adjoint_1d", src, out, P, Lo, Li, Q, sp, so, a1, a2, 1.0, dtype_code(src), dtype_code(out))
    return out


def decoder_fuse_fwd(e1, Wc1, bias, zs, H1, W1, hw):
    """Z (B*N1, E) = e1 Wc1^T + bias + up(zs[0]) + up(zs[1]) + up(zs[2]) (cmx_decoder_fuse_fwd: the upsample of the
    c4, c3, c2 products, grids hw[2], hw[1], hw[0], in the c1 GEMM's epilogue); e1 (B, N1, K) contiguous, Wc1 (E, K)."""
    B, N1, Kd = e1.shape
    E = Wc1.shape[0]
    Z = torch.empty(B * N1, E, dtype=e1.dtype, device=e1.device)
    call("cmx_decoder_fuse_fwd", e1, Wc1, Z, bias, zs[0], zs[1], zs[2], B, H1, W1, *hw[2], *hw[1], *hw[0], E, Kd, Kd,
         Wc1.stride(0), dtype_code(e1))
    return Z


# ------------------------------------------------------------------------------ eASPP neck (include/cmx_easpp.h)
def easpp_conv(entry: str, a, Ws, out, B, h, w, rates):
    """cmx_easpp_conv_fwd / cmx_easpp_conv_dgrad (``entry``) on the three branches' rows a[g] (B*h*w, 64 at any row
    stride), tap-major weights Ws[g] (64, 3, 3, 64) and outputs out[g] (the caller's)."""
    call(entry, *a, *Ws, *out, B, h, w, a[0].shape[-1], *rates, a[0].stride(0), out[0].stride(0), dtype_code(a[0]))
    return out


def easpp_conv_wgrad(dys, xs, Wgs, B, h, w, rates):
    """Wgs[g] (fp32 (64, 3, 3, 64) views of the gradient buffer) = the branches' weight gradients (overwritten)."""
    ws = _ws(query("cmx_easpp_conv_wgrad_workspace", B, h, w), xs[0].device)
    call("cmx_easpp_conv_wgrad", *dys, *xs, *Wgs, ws, B, h, w, xs[0].shape[-1], *rates, dys[0].stride(0),
         xs[0].stride(0), dtype_code(xs[0]))


# ------------------------------------------------------------------------------ DeepLabV3+ head (include/cmx_deeplab.h)
def aspp_conv_fwd(x, Ws, B, h, w, rates):
    """ASPP's three dilated 3x3 convolutions of ONE input x (B*h*w, Cin at any row stride) with the tap-major weights
    Ws[g] (Cout, 3, 3, Cin): the three outputs (B*h*w, Cout) of one launch (cmx_aspp_conv_fwd)."""
    Cout, Cin = Ws[0].shape[0], Ws[0].shape[-1]
    ys = tuple(torch.empty(x.shape[0], Cout, dtype=x.dtype, device=x.device) for _ in range(3))
    call("cmx_aspp_conv_fwd", x, *Ws, *ys, B, h, w, Cin, Cout, *rates, x.stride(0), Cout, dtype_code(x))
    return ys


def aspp_conv_dgrad(dys, Ws, B, h, w, rates):
    """dx (B*h*w, Cin): the SUM of the three branches' input gradients, rounded once (cmx_aspp_conv_dgrad); the three
    dys[g] (B*h*w, Cout) share one row stride."""
    Cout, Cin = Ws[0].shape[0], Ws[0].shape[-1]
    dx = torch.empty(dys[0].shape[0], Cin, dtype=dys[0].dtype, device=dys[0].device)
    call("cmx_aspp_conv_dgrad", *dys, *Ws, dx, B, h, w, Cin, Cout, *rates, dys[0].stride(0), Cin, dtype_code(dx))
    return dx


def aspp_conv_wgrad(dys, x, Wgs, B, h, w, rates):
    """Wgs[g] (fp32 (Cout, 3, 3, Cin) views of the gradient buffer) = the branches' weight gradients (overwritten)."""
    Cout, Cin = Wgs[0].shape[0], Wgs[0].shape[-1]
    ws = _ws(query("cmx_aspp_conv_wgrad_workspace", B, h, w, Cin, Cout), x.device)
    call("cmx_aspp_conv_wgrad", *dys, x, *Wgs, ws, B, h, w, Cin, Cout, *rates, dys[0].stride(0), x.stride(0),
         dtype_code(x))


def upcat_ac_fwd(lo, skip, B, h, w, H, W):
    """cat (B*H*W, C + Cs) = [bilinear align_corners=True upsample of lo (B*h*w, C) | skip (B*H*W, Cs)], contiguous
    operands (cmx_upcat_ac_fwd)."""
    C, Cs = lo.shape[-1], skip.shape[-1]
    cat = torch.empty(B * H * W, C + Cs, dtype=lo.dtype, device=lo.device)
    call("cmx_upcat_ac_fwd", lo, skip, cat, B, h, w, H, W, C, Cs, dtype_code(lo))
    return cat


def upcat_ac_bwd(dcat, B, h, w, H, W, C, Cs):
    """(dlo (B*h*w, C), dskip (B*H*W, Cs)) of upcat_ac_fwd, one launch (cmx_upcat_ac_bwd)."""
    dlo = torch.empty(B * h * w, C, dtype=dcat.dtype, device=dcat.device)
    dskip = torch.empty(B * H * W, Cs, dtype=dcat.dtype, device=dcat.device)
    call("cmx_upcat_ac_bwd", dcat, dlo, dskip, B, h, w, H, W, C, Cs, dtype_code(dcat))
    return dlo, dskip


# ------------------------------------------------------------------------------ UPerNet head (include/cmx_uper.h)
def ppm_rows(scales) -> int:
    """Pooled rows per image of the pyramid pooling at ``scales``: sum of s^2."""
    return sum(s * s for s in scales)


def _scales4(scales):
    scales = tuple(int(s) for s in scales)
    return scales + (0,) * (4 - len(scales))


def ppm_pool_fwd(x, B, h, w, scales):
    """pooled (B * sum s^2, C): nn.AdaptiveAvgPool2d(s) of x (B*h*w, C) at up to four scales, one launch; block k
    starts at row B * sum_{j<k} s_j^2 and holds (B, s_k, s_k, C) (cmx_ppm_pool_fwd)."""
    C = x.shape[-1]
    pooled = torch.empty(B * ppm_rows(scales), C, dtype=x.dtype, device=x.device)
    call("cmx_ppm_pool_fwd", x, pooled, B, h, w, C, *_scales4(scales), dtype_code(x))
    return pooled


def ppm_pool_bwd(dpooled, add, B, h, w, scales):
    """dx (B*h*w, C) of ppm_pool_fwd on top of ``add`` (B*h*w rows of C at any row stride, or None), one launch
    (cmx_ppm_pool_bwd)."""
    C = dpooled.shape[-1]
    dx = torch.empty(B * h * w, C, dtype=dpooled.dtype, device=dpooled.device)
    call("cmx_ppm_pool_bwd", dpooled, add, add.stride(0) if add is not None else 0, dx, B, h, w, C, *_scales4(scales),
         dtype_code(dpooled))
    return dx


def _grids4(grids):
    flat = [int(v) for g in grids for v in g]
    return flat + [0] * (8 - len(flat))


def upcat_multi_fwd(skip, srcs, B, H, W, grids):
    """cat (B*H*W, Cs + n*C) = [skip | up(srcs[0]) | ...], bilinear align_corners=False from the sources' own grids
    ``grids`` = ((h_i, w_i), ...), contiguous operands, one launch (cmx_upcat_multi_fwd); skip None: Cs = 0."""
    n, C = len(srcs), srcs[0].shape[-1]
    Cs = skip.shape[-1] if skip is not None else 0
    cat = torch.empty(B * H * W, Cs + n * C, dtype=srcs[0].dtype, device=srcs[0].device)
    ps = list(srcs) + [None] * (4 - n)
    call("cmx_upcat_multi_fwd", skip, *ps, cat, B, H, W, Cs, C, n, *_grids4(grids), dtype_code(cat))
    return cat


def upcat_multi_bwd(dcat, B, H, W, Cs, C, grids, want_skip=True):
    """(dskip (B*H*W, Cs) or None, [dsrc_i (B*h_i*w_i, C)]) of upcat_multi_fwd, one launch (cmx_upcat_multi_bwd)."""
    n = len(grids)
    dskip = torch.empty(B * H * W, Cs, dtype=dcat.dtype, device=dcat.device) if (want_skip and Cs > 0) else None
    ds = [torch.empty(B * h * w, C, dtype=dcat.dtype, device=dcat.device) for h, w in grids]
    call("cmx_upcat_multi_bwd", dcat, dskip, *(ds + [None] * (4 - n)), B, H, W, Cs, C, n, *_grids4(grids),
         dtype_code(dcat))
    return dskip, ds


def up_add_fwd(hi, lo, B, h, w, H, W):
    """hi (B*H*W, C) + the bilinear align_corners=False upsample of lo (B*h*w, C), in a new tensor (cmx_up_add_fwd)."""
    out = torch.empty_like(hi)
    call("cmx_up_add_fwd", hi, lo, out, B, h, w, H, W, hi.shape[-1], dtype_code(hi))
    return out


def conv_flip_weight(W, KH, KW, C):
    """Wf (G, C, KH*KW*N) with Wf[g][ci][T - 1 - t][co] = W[g][co][t][ci] from the 16-bit tap-major weights W
    (G, N, KH*KW*C) (cmx_conv_flip_weight, one launch per group): the weights whose stride-1 'same' convolution with
    dy is the input gradient."""
    G, N = W.shape[:2]
    Wf = torch.empty(G, C, KH * KW * N, dtype=W.dtype, device=W.device)
    for g in range(G):
        call("cmx_conv_flip_weight", W[g], Wf[g], N, KH, KW, C, W.stride(1), dtype_code(W))
    return Wf
