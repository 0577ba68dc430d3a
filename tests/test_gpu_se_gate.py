"""The four channel-attention gate kernels (csrc/se_gate.hip) through the C-ABI.

Every device buffer sits between guards of a NaN bit pattern (a stray write shows in the guard, a
stray read in the arithmetic).  Shapes: B in {1, 3}, C in {8 (one 16-bit vector), 256, 768 (three
column tiles)}, N in {1, 77, one row chunk + 1, three chunks + 5 (four partials to fold)}; the
chunk size is the kernel's own (cmx_se_chunk_rows).

* Gaussian inputs against fp64: |err| <= 2 E_emul + u max|ref|, E_emul = the error of the same
  formula evaluated by torch in fp32 on the same (storage-rounded) inputs, u = the unit roundoff of
  the output's storage type.
* small integers with power-of-two a / dscale (0 = a dropped channel included): every sum and
  product is exact, so scale / apply outputs are torch.equal to the reference and pooled / da are
  within one fp32 ulp of fl(sum / N) / fl(sum).
* dscale = NULL, determinism (two launches bit-equal, tickets zero after each), refusals, and the
  hand-off to cmx_small_linear_bwd in both directions.
"""
import functools
import itertools
import os
import sys

import pytest
import torch

from rgbx_semantic_segmentation_amd import _lib
from rgbx_semantic_segmentation_amd._lib import call, ptr, query, stream, try_call

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_harness import CODE, Guarded  # noqa: E402

pytestmark = pytest.mark.gpu

UNIT = {torch.float32: 2.0 ** -23, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -10}
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
ROWS = query("cmx_se_chunk_rows")
NS = (1, 77, ROWS + 1, 3 * ROWS + 5)
SHAPES = [(B, N, C) for B, C, N in itertools.product((1, 3), (8, 256, 768), NS)]
SHAPE_IDS = [f"B{B}-N{N}-C{C}" for B, N, C in SHAPES]
FEW = [(1, 3 * ROWS + 5, 768), (3, ROWS + 1, 256), (3, 77, 8)]
FEW_IDS = [f"B{B}-N{N}-C{C}" for B, N, C in FEW]
NSL = query("cmx_small_linear_nslice")


class Gate:
    """One problem on the device: guarded inputs, guarded outputs, the four launches."""

    def __init__(self, dev, dtype, B, N, C, y, dout, a, ds, part):
        self.dtype, self.B, self.N, self.C, self.dt = dtype, B, N, C, CODE[dtype]
        self.y = Guarded((B, N, C), dtype, dev, y)
        self.dout = Guarded((B, N, C), dtype, dev, dout)
        self.a = Guarded((B, C), torch.float32, dev, a)
        self.ds = Guarded((B, C), torch.float32, dev, ds) if ds is not None else None
        self.part = Guarded(tuple(part.shape), torch.float32, dev, part)
        self.nz = query("cmx_se_pool_nchunk", B, N, C)
        self.nda = query("cmx_se_bwd_nslice", B, N, C)
        self.pooled = Guarded((B, C), torch.float32, dev)
        self.ws = Guarded((query("cmx_se_pool_workspace", B, N, C) // 4,), torch.float32, dev)
        self.tk = Guarded((query("cmx_se_pool_tickets", B, C),), torch.int32, dev,
                          torch.zeros(query("cmx_se_pool_tickets", B, C), dtype=torch.int32))
        self.out = Guarded((B, N, C), dtype, dev)
        self.dap = Guarded((self.nda, B, C), torch.float32, dev)
        self.dy = Guarded((B, N, C), dtype, dev)
        self.bufs = [self.y, self.dout, self.a, self.part, self.pooled, self.ws, self.tk, self.out, self.dap,
                     self.dy]
        if self.ds is not None:
            self.bufs.append(self.ds)

    def launch(self):
        B, N, C, dt = self.B, self.N, self.C, self.dt
        dsp = ptr(self.ds.t) if self.ds is not None else 0
        call("cmx_se_pool_fwd", ptr(self.y.t), ptr(self.pooled.t), ptr(self.ws.t), ptr(self.tk.t), B, N, C, dt, stream())
        call("cmx_se_scale_fwd", ptr(self.y.t), ptr(self.a.t), dsp, ptr(self.out.t), B, N, C, dt, stream())
        call("cmx_se_bwd_reduce", ptr(self.dout.t), ptr(self.y.t), dsp, ptr(self.dap.t), B, N, C, dt, stream())
        call("cmx_se_bwd_apply", ptr(self.dout.t), ptr(self.a.t), dsp, ptr(self.part.t), self.part.t.shape[0], B * C,
             ptr(self.dy.t), B, N, C, dt, stream())
        torch.cuda.synchronize()
        assert all(b.intact() for b in self.bufs), "a guard changed"
        assert not bool(self.tk.t.any()), "tickets not left at zero"
        return (self.pooled.t.cpu(), self.out.t.cpu(), self.dap.t.cpu(), self.dy.t.cpu())


def _formula(y, dout, a, ds, part, N):
    """(pooled, out, da, dy) in the dtype of the arguments (fp64: the reference; fp32: the emulation)."""
    f = a if ds is None else a * ds
    pooled = y.sum(1) / N
    out = y * f[:, None, :]
    da = (dout * y).sum(1)
    if ds is not None:
        da = da * ds
    dy = dout * f[:, None, :] + (part.sum(0) / N)[:, None, :]
    return pooled, out, da, dy


@functools.lru_cache(maxsize=None)
def _gauss(dtype, B, N, C, null):
    """Inputs rounded to their storage type, the fp64 reference of them and the bounds."""
    g = torch.Generator().manual_seed(1000 * B + 7 * N + C)
    y = (0.25 + torch.randn(B, N, C, generator=g)).to(dtype)
    dout = (0.1 * torch.randn(B, N, C, generator=g)).to(dtype)
    a = torch.sigmoid(torch.randn(B, C, generator=g))
    ds = None if null else (torch.rand(B, C, generator=g) > 0.2).float() / 0.9
    part = torch.randn(NSL - 3, B, C, generator=g)          # fewer slices than the kernel's maximum
    dbl = lambda t: None if t is None else t.double()
    ref = _formula(dbl(y), dbl(dout), dbl(a), dbl(ds), dbl(part), N)
    emu = _formula(y.float(), dout.float(), a, ds, part, N)
    bounds = []
    for r, e, u in zip(ref, emu, (UNIT[torch.float32], UNIT[dtype], UNIT[torch.float32], UNIT[dtype])):
        bounds.append(2 * (e.double() - r).abs().max().item() + u * r.abs().max().item())
    return (y, dout, a, ds, part), ref, bounds


@pytest.mark.parametrize("null", [False, True], ids=["dscale", "null"])
@pytest.mark.parametrize("B,N,C", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_gaussian_against_fp64(dev, dtype, B, N, C, null):
    ins, ref, bounds = _gauss(dtype, B, N, C, null)
    got = Gate(dev, dtype, B, N, C, *ins).launch()
    got = (got[0], got[1], got[2].double().sum(0), got[3])       # da: the slices summed on the host in fp64
    for name, g, r, bound in zip(("pooled", "out", "da", "dy"), got, ref, bounds):
        err = (g.double() - r).abs().max().item()
        print(f"{name}: err {err:.3e} bound {bound:.3e}")
        assert err <= bound, (name, err, bound)


@functools.lru_cache(maxsize=None)
def _ints(B, N, C):
    g = torch.Generator().manual_seed(5 + 1000 * B + 7 * N + C)
    y = torch.randint(-3, 4, (B, N, C), generator=g).double()
    dout = torch.randint(-3, 4, (B, N, C), generator=g).double()
    a = 2.0 ** torch.randint(-1, 2, (B, C), generator=g).double()
    ds = torch.tensor([0.0, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (B, C), generator=g)]
    # NSL slices of multiples of N that sum to N * k, |k| <= 2: part.sum(0) / N = k exactly
    k = torch.randint(-2, 3, (B, C), generator=g).double()
    part = N * torch.randint(-2, 3, (NSL, B, C), generator=g).double()
    part[0] += N * k - part.sum(0)
    return y, dout, a, ds, part


@pytest.mark.parametrize("null", [False, True], ids=["dscale", "null"])
@pytest.mark.parametrize("B,N,C", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_on_small_integers(dev, dtype, B, N, C, null):
    y, dout, a, ds, part = _ints(B, N, C)
    if null:
        ds = None
    pooled, out, da, dy = _formula(y, dout, a, ds, part, N)
    assert torch.equal(out.to(dtype).double(), out) and torch.equal(dy.to(dtype).double(), dy)   # representable
    f32 = lambda t: None if t is None else t.float()
    g_pooled, g_out, g_dap, g_dy = Gate(dev, dtype, B, N, C, y.to(dtype), dout.to(dtype), f32(a), f32(ds),
                                        f32(part)).launch()
    assert torch.equal(g_out, out.to(dtype))
    assert torch.equal(g_dy, dy.to(dtype))
    want = (y.sum(1) / N).float()                             # fl(sum / N): the sum itself is exact
    ulp = torch.maximum(want.abs(), torch.tensor(2.0 ** -126)).log2().floor().exp2() * 2.0 ** -23
    assert bool(((g_pooled - want).abs() <= ulp).all())
    # every slice is an exact integer, so their fp64 sum is the kernel's da exactly
    assert torch.equal(g_dap.double().sum(0), da)


@pytest.mark.parametrize("B,N,C", FEW, ids=FEW_IDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_two_launches_bit_equal(dev, dtype, B, N, C):
    ins, _, _ = _gauss(dtype, B, N, C, False)
    gate = Gate(dev, dtype, B, N, C, *ins)
    first = [t.clone() for t in gate.launch()]                 # launch() checks the tickets after each
    gate.ws.t.fill_(float("nan"))                              # the partials of the first launch are not reused
    second = gate.launch()
    for u, v in zip(first, second):
        assert torch.equal(u.view(torch.uint8), v.view(torch.uint8))


def test_refusals(dev):
    """Bad shapes and missing buffers return a status (nothing is launched)."""
    t = torch.zeros(4096, device=dev)
    tk = torch.zeros(64, dtype=torch.int32, device=dev)
    s = stream()
    assert try_call("cmx_se_pool_fwd", ptr(t), ptr(t), ptr(t), ptr(tk), 1, 4, 12, 0, s) == _lib.CMX_ERR_SHAPE
    assert try_call("cmx_se_pool_fwd", ptr(t), ptr(t), ptr(t), 0, 1, 4, 16, 0, s) == _lib.CMX_ERR_ARG
    assert try_call("cmx_se_pool_fwd", ptr(t), ptr(t), ptr(t), ptr(tk), 1, 4, 16, 7, s) == _lib.CMX_ERR_DTYPE
    assert try_call("cmx_se_scale_fwd", ptr(t), ptr(t), 0, ptr(t), 0, 4, 16, 0, s) == _lib.CMX_ERR_SHAPE
    assert try_call("cmx_se_scale_fwd", ptr(t), ptr(t) + 4, 0, ptr(t), 1, 4, 16, 0, s) == _lib.CMX_ERR_ARG
    assert try_call("cmx_se_bwd_reduce", ptr(t), ptr(t), 0, 0, 1, 4, 16, 0, s) == _lib.CMX_ERR_ARG
    assert try_call("cmx_se_bwd_apply", ptr(t), ptr(t), 0, ptr(t), NSL + 1, 16, ptr(t), 1, 4, 16, 0, s) \
        == _lib.CMX_ERR_SHAPE
    torch.cuda.synchronize()
    assert not bool(tk.any())


# ------------------------------------------------------------------ hand-off to cmx_small_linear_bwd
def _linear_bwd(dy_part, nslice, ss, rs, yout, x, w, M, Kin, Nout, act, dev, want_dx=True):
    dw = torch.full((Nout, Kin), float("nan"), device=dev)
    db = torch.full((Nout,), float("nan"), device=dev)
    dxp = torch.full((NSL, M, Kin), float("nan"), device=dev) if want_dx else None
    call("cmx_small_linear_bwd", ptr(dy_part), nslice, ss, rs, ptr(yout), ptr(x), ptr(w), ptr(dxp), ptr(dw), ptr(db), M,
         Kin, Nout, act, 0, stream())
    return dw, db, dxp


@pytest.mark.parametrize("exact", [True, False], ids=["ints", "gauss"])
@pytest.mark.parametrize("B,C", [(1, 256), (3, 768)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_reduce_slices_feed_the_gemv_backward(dev, dtype, B, C, exact):
    """cmx_se_bwd_reduce's slices as cmx_small_linear_bwd's dy_part give the dw / db / dx of feeding
    it the summed da as one slice: equal bits on integer data (every sum exact), and on Gaussian data
    both within the fp32 bound of the fp64 gradient."""
    N, H = 3 * ROWS + 5, C // 4
    if exact:
        y, dout, _, ds, _ = _ints(B, N, C)
    else:
        (y, dout, _, ds, _), _, _ = _gauss(dtype, B, N, C, False)
    g = torch.Generator().manual_seed(9)
    if exact:                                                    # a = 1/2: act' = a (1 - a) = 1/4
        aout = torch.full((B, C), 0.5)
        h1 = torch.randint(-2, 3, (B, H), generator=g).float()
        W2 = torch.randint(-2, 3, (C, H), generator=g).float()
    else:
        aout = torch.sigmoid(torch.randn(B, C, generator=g))
        h1, W2 = torch.randn(B, H, generator=g), torch.randn(C, H, generator=g) / H ** 0.5
    yd, dd = y.to(dtype).to(dev), dout.to(dtype).to(dev)
    dsd = ds.float().to(dev)
    nda = query("cmx_se_bwd_nslice", B, N, C)
    assert nda >= 3
    dap = torch.full((nda, B, C), float("nan"), device=dev)
    call("cmx_se_bwd_reduce", ptr(dd), ptr(yd), ptr(dsd), ptr(dap), B, N, C, CODE[dtype], stream())
    ad, hd, wd = aout.to(dev), h1.to(dev), W2.to(dev)
    sliced = _linear_bwd(dap, nda, B * C, C, ad, hd, wd, B, H, C, 3, dev)
    da1 = dap.double().sum(0).float().contiguous()
    single = _linear_bwd(da1, 1, 0, C, ad, hd, wd, B, H, C, 3, dev)
    torch.cuda.synchronize()
    da64 = (dd.double() * yd.double()).sum(1).cpu() * ds.double()
    dz = da64 * (aout.double() * (1 - aout.double()))
    refs = (dz.t() @ h1.double(), dz.sum(0), dz @ W2.double())
    dz32 = (da64.float() * (aout * (1 - aout)))
    emus = (dz32.t() @ h1, dz32.sum(0), dz32 @ W2)
    for name, s, o, r, e in zip(("dw", "db", "dx"), sliced, single, refs, emus):
        if name == "dx":
            s, o = s.double().sum(0), o.double().sum(0)
        if exact:
            assert torch.equal(s.cpu().double(), r) and torch.equal(o.cpu().double(), r), name
        else:
            bound = 2 * (e.double() - r).abs().max().item() + UNIT[torch.float32] * r.abs().max().item()
            for v in (s, o):
                assert (v.cpu().double() - r).abs().max().item() <= bound, name


@pytest.mark.parametrize("B,C", [(1, 256), (3, 768)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_apply_sums_the_gemv_backward_slices(dev, dtype, B, C):
    """cmx_se_bwd_apply on the dx slices cmx_small_linear_bwd really writes: with dout = 0 its output is
    the pooled-gradient term (dz1 W1) / N of every row, against fp64."""
    N, H = 77, C // 4
    g = torch.Generator().manual_seed(11)
    dz1, W1 = torch.randn(B, H, generator=g), torch.randn(H, C, generator=g) / C ** 0.5
    pooled, z1 = torch.randn(B, C, generator=g), torch.randn(B, H, generator=g)
    _, _, dxp = _linear_bwd(dz1.to(dev), 1, 0, H, z1.to(dev), pooled.to(dev), W1.to(dev), B, C, H, 0, dev)
    a = torch.ones(B, C, device=dev)
    dout = torch.zeros(B, N, C, dtype=dtype, device=dev)
    dy = torch.full((B, N, C), float("nan"), dtype=dtype, device=dev)
    call("cmx_se_bwd_apply", ptr(dout), ptr(a), 0, ptr(dxp), NSL, B * C, ptr(dy), B, N, C, CODE[dtype], stream())
    torch.cuda.synchronize()
    ref = (dz1.double() @ W1.double()) / N
    emu = (dz1 @ W1) / N
    bound = 2 * (emu.double() - ref).abs().max().item() + UNIT[dtype] * ref.abs().max().item()
    got = dy.cpu().double()
    assert torch.equal(got, got[:, :1].expand_as(got))        # the same term on every row
    assert (got[:, 0] - ref).abs().max().item() <= bound
