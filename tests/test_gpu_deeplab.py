"""The DeepLabV3+ decode head on the GPU.

1. The wide grouped dilated 3x3 convolution alone, through the C-ABI (cmx_aspp_conv_fwd / _dgrad / _wgrad), by the
   method of tests/test_gpu_easpp.py, against torch.nn.functional.conv2d(dilation=r, padding=r) in fp64 on the CPU; the
   input gradient is the SUM of the three branches' references.  Exact draw (0/1 activations, -1/0/1 weights in a band
   of width 9: |y| <= 81, |sum_g dx| <= 243, dw an integer below 2^24): bit-equal in all three dtypes.  Dyadic grid draw
   (activations in multiples of 1/8, weights of 1/64 up to 1/4): every partial sum is exact in fp32, so dw and the fp32
   outputs are bit-equal and a 16-bit output is the fp64 result rounded to the type, bit for bit.  Normal draw: dw and
   fp32 outputs within 4x the error of torch's own fp32 CPU conv2d; 16-bit outputs to one unit in the last place or
   that fp32 rule (test_gpu_easpp.py::test_conv_random).  Outputs sit in sentinel-filled buffers with row stride > C and
   guard rows.
2. The align-corners upsample + concat alone (cmx_upcat_ac_fwd / _bwd) against F.interpolate(align_corners=True) +
   cat and autograd in fp64.
3. The head alone (DeepLabV3Plus.run) against the fp64 restatement tests/deeplab_ref.py, by the method and margins of
   tests/test_gpu_fcn_head.py item 1.
4. The two random dropout masks (kept share, scale, fresh on graph replay, none in eval mode, a first draw inside a
   capture raises).
5. The whole model (mit_b0, K = 9, B = 2, fp32, forced masks) at 64 x 96 and 64 x 416, with the default auxiliary head
   and without it, and once with DiceCELoss, against the fp64 oracle carrying the restated heads, with
   tests/test_gpu_easpp.py::test_model_train_step_fp32's bounds; no head tensor among the outliers.  The HEAD's ReLU
   kinks are settled on the CPU first (_settle_head says why).
6. One bf16 training step with the auxiliary head captured in a HIP graph and replayed twice: bit-equal to eager.
7. train.py --decoder DeepLabV3Plus end to end; a reference-format checkpoint loads strictly.
"""
import copy
import functools
import gc
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as TF

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import dice_cases as dc  # noqa: E402
from deeplab_ref import DeepLabV3PlusRef, jitter, ref_model, settle_kinks  # noqa: E402
from oracle.bf16_emul import emulate_storage  # noqa: E402
from test_config_parity import _masks  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
GUARD, PADX, PADY = 3, 8, 16
# (B, h, w), rates, (Cin, Cout): centre taps only with M = 6 below one tile; all nine taps, every border, M = 70 no tile
# multiple; rate 12 reaches both axes / 24 only x / 36 neither (three row chunks); offset = size - 1 and a Cout that is
# no power of two (two row chunks); the mit_b2 training map
CONV_CASES = [((1, 2, 3), (12, 24, 36), (256, 256)), ((2, 5, 7), (1, 2, 3), (128, 64)),
              ((2, 14, 26), (12, 24, 36), (64, 128)), ((3, 13, 25), (12, 24, 12), (128, 192)),
              ((1, 15, 20), (12, 24, 36), (512, 256))]
CONV_IDS = ["a_2x3", "b_5x7_r123", "c_14x26", "d_13x25_edge", "e_15x20"]


# ------------------------------------------------------------------ 1. the grouped convolution alone
def _draw(kind, shape, chans, seed):
    """x (B, Cin, h, w) and per branch w (Cout, Cin, 3, 3), dy (B, Cout, h, w), fp64."""
    (B, h, w), (Cin, Cout) = shape, chans
    g = torch.Generator().manual_seed(seed)
    ws, dys = [], []
    if kind == "exact":
        x = (torch.rand(B, Cin, h, w, generator=g) < 0.5).double()
    elif kind == "grid":
        x = torch.randint(-8, 9, (B, Cin, h, w), generator=g).double() / 8
    else:
        x = torch.randn(B, Cin, h, w, generator=g).double()
    for _ in range(3):
        if kind == "exact":
            dy = (torch.rand(B, Cout, h, w, generator=g) < 0.5).double()
            co, ci = torch.arange(Cout)[:, None, None], torch.arange(Cin)[None, :, None]
            tap = torch.arange(9)[None, None, :]
            band = ((ci - co - 7 * tap) % max(Cin, Cout)) < 9     # at most 9 per row and per column of every tap
            wt = torch.randint(-1, 2, (Cout, Cin, 9), generator=g).double() * band
            assert int((wt != 0).sum(1).max()) <= 9 and int((wt != 0).sum(0).max()) <= 9
            wt = wt.view(Cout, Cin, 3, 3)
        elif kind == "grid":
            dy = torch.randint(-8, 9, (B, Cout, h, w), generator=g).double() / 8
            wt = torch.randint(-16, 17, (Cout, Cin, 3, 3), generator=g).double() / 64
        else:
            dy = torch.randn(B, Cout, h, w, generator=g).double()
            wt = torch.randn(Cout, Cin, 3, 3, generator=g).double() * (2.0 / (9 * Cin)) ** 0.5
        ws.append(wt), dys.append(dy)
    return x, ws, dys


@functools.lru_cache(maxsize=None)
def _conv_ref(kind, shape, rates, chans, dtype, seed=0):
    """Inputs (rounded to ``dtype``) and fp64 results (dx: summed over the branches); e32: torch's fp32 CPU errors."""
    x, ws, dys = _draw(kind, shape, chans, seed)
    rnd = lambda t: t.to(dtype).double()
    x, ws, dys = rnd(x), [rnd(t) for t in ws], [rnd(t) for t in dys]
    res = {}
    for ft in (torch.float64, torch.float32):
        xi = x.to(ft).clone().requires_grad_(True)
        wi = [t.to(ft).clone().requires_grad_(True) for t in ws]
        ys = [TF.conv2d(xi, wt, dilation=r, padding=r) for wt, r in zip(wi, rates)]
        torch.autograd.backward(ys, [d.to(ft) for d in dys])
        res[ft] = ([y.detach().double() for y in ys], xi.grad.double(), [t.grad.double() for t in wi])
    a, b = res[torch.float64], res[torch.float32]
    e32 = {"y": max((p - q).abs().max().item() for p, q in zip(a[0], b[0])), "dx": (a[1] - b[1]).abs().max().item(),
           "dw": max((p - q).abs().max().item() for p, q in zip(a[2], b[2]))}
    return {"x": x, "w": ws, "dy": dys, "y": a[0], "dx": a[1], "dw": a[2], "e32": e32}


def _rows(t):
    """NCHW (B, C, h, w) -> token-major rows (B*h*w, C)."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _nchw(rows, shape):
    B, h, w = shape
    return rows.reshape(B, h, w, -1).permute(0, 3, 1, 2)


def _bits(t):
    return t.view({4: torch.int32, 2: torch.int16}[t.element_size()])


def _padded(ts, M, C, ld, dtype, dev, sentinel=-777.0):
    """len(ts) (M, C) tensors (None: left as sentinel) inside one sentinel-filled (n, GUARD + M + GUARD, ld) buffer."""
    buf = torch.full((len(ts), M + 2 * GUARD, ld), sentinel, dtype=dtype, device=dev)
    views = [buf[g, GUARD:GUARD + M, :C] for g in range(len(ts))]
    for v, t in zip(views, ts):
        if t is not None:
            v.copy_(t.to(dtype))
    return buf, views


def _untouched(buf, before, M, C):
    keep = torch.ones_like(buf, dtype=torch.bool)
    keep[:, GUARD:GUARD + M, :C] = False
    return torch.equal(_bits(buf)[keep], _bits(before)[keep])


def _run_conv(ref, shape, rates, chans, dtype, dev):
    """fwd, dgrad, wgrad (twice) through the C-ABI on strided, guarded buffers -> (y list, dx, dw list) as fp64 CPU
    tensors (NCHW / (Cout, Cin, 3, 3)), after checking that nothing outside the results changed."""
    from rgbx_semantic_segmentation_amd import _lib
    (B, h, w), (Cin, Cout) = shape, chans
    M, wsz = B * h * w, Cout * 9 * Cin
    code = _lib.DTYPE_CODES[dtype]
    _, (xv,) = _padded([_rows(ref["x"])], M, Cin, Cin + PADX, dtype, dev)
    _, dyv = _padded([_rows(t) for t in ref["dy"]], M, Cout, Cout + PADX, dtype, dev)
    wt = [t.permute(0, 2, 3, 1).contiguous().to(dtype).to(dev) for t in ref["w"]]       # tap-major (Cout, kh, kw, Cin)
    ybuf, yv = _padded([None] * 3, M, Cout, Cout + PADY, dtype, dev)
    dxbuf, (dxv,) = _padded([None], M, Cin, Cin + PADY, dtype, dev)
    dwbuf = torch.full((3, wsz + 2 * 64), -777.0, dtype=torch.float32, device=dev)
    dwv = [dwbuf[g, 64:64 + wsz] for g in range(3)]
    y0, dx0, dw0 = ybuf.clone(), dxbuf.clone(), dwbuf.clone()
    _lib.call("cmx_aspp_conv_fwd", xv, *wt, *yv, B, h, w, Cin, Cout, *rates, Cin + PADX, Cout + PADY, code)
    _lib.call("cmx_aspp_conv_dgrad", *dyv, *wt, dxv, B, h, w, Cin, Cout, *rates, Cout + PADX, Cin + PADY, code)
    nws = _lib.query("cmx_aspp_conv_wgrad_workspace", B, h, w, Cin, Cout)
    ws = torch.full((max(1, nws // 4),), float("nan"), dtype=torch.float32, device=dev)
    wg = (*dyv, xv, *dwv, ws, B, h, w, Cin, Cout, *rates, Cout + PADX, Cin + PADX, code)
    _lib.call("cmx_aspp_conv_wgrad", *wg)
    first = dwbuf.clone()
    _lib.call("cmx_aspp_conv_wgrad", *wg)
    torch.cuda.synchronize()
    assert torch.equal(_bits(first), _bits(dwbuf)), "the weight gradient differs from run to run"
    assert _untouched(ybuf, y0, M, Cout), "forward wrote outside its outputs"
    assert _untouched(dxbuf, dx0, M, Cin), "dgrad wrote outside its outputs"
    edge = torch.ones_like(dwbuf, dtype=torch.bool)
    edge[:, 64:64 + wsz] = False
    assert torch.equal(dwbuf[edge], dw0[edge]), "wgrad wrote outside its outputs"
    y = [_nchw(v.double().cpu(), shape) for v in yv]
    dx = _nchw(dxv.double().cpu(), shape)
    dw = [v.view(Cout, 3, 3, Cin).permute(0, 3, 1, 2).double().cpu() for v in dwv]
    return y, dx, dw


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,rates,chans", CONV_CASES, ids=CONV_IDS)
def test_conv_exact(dev, shape, rates, chans, dtype):
    ref = _conv_ref("exact", shape, rates, chans, torch.float64)
    assert max(t.abs().max().item() for t in ref["y"]) <= 81 and ref["dx"].abs().max().item() <= 243
    assert max(t.abs().max().item() for t in ref["dw"]) < 2 ** 24
    y, dx, dw = _run_conv(ref, shape, rates, chans, dtype, dev)
    assert torch.equal(dx, ref["dx"]), (dx - ref["dx"]).abs().max().item()
    for g in range(3):
        assert torch.equal(y[g], ref["y"][g]), ("y", g, (y[g] - ref["y"][g]).abs().max().item())
        assert torch.equal(dw[g], ref["dw"][g]), ("dw", g, (dw[g] - ref["dw"][g]).abs().max().item())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,rates,chans", CONV_CASES, ids=CONV_IDS)
def test_conv_grid(dev, shape, rates, chans, dtype):
    ref = _conv_ref("grid", shape, rates, chans, torch.float64)
    y, dx, dw = _run_conv(ref, shape, rates, chans, dtype, dev)
    rnd = lambda t: t.to(dtype).double()               # fp32: every sum of the grid is exact, so this is the identity
    assert torch.equal(dx, rnd(ref["dx"])), (dx - rnd(ref["dx"])).abs().max().item()
    for g in range(3):
        assert torch.equal(y[g], rnd(ref["y"][g])), ("y", g, (y[g] - rnd(ref["y"][g])).abs().max().item())
        assert torch.equal(dw[g], ref["dw"][g]), ("dw", g, (dw[g] - ref["dw"][g]).abs().max().item())


def _ulp_dist(a, b, dtype):
    """Elementwise distance of a and b (both representable in the 16-bit ``dtype``) in units in the last place."""
    def ordinal(t):
        i = t.to(dtype).view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (ordinal(a) - ordinal(b)).abs()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,rates,chans", CONV_CASES, ids=CONV_IDS)
def test_conv_random(dev, shape, rates, chans, dtype):
    ref = _conv_ref("normal", shape, rates, chans, dtype)
    y, dx, dw = _run_conv(ref, shape, rates, chans, dtype, dev)
    e32 = ref["e32"]
    err = {"y": max((a - b).abs().max().item() for a, b in zip(y, ref["y"])), "dx": (dx - ref["dx"]).abs().max().item(),
           "dw": max((a - b).abs().max().item() for a, b in zip(dw, ref["dw"]))}
    print(f"aspp conv random {dtype} {shape} {rates} {chans}: err {err} torch-fp32 {e32}")
    assert err["dw"] <= 4 * e32["dw"], (err, e32)
    if dtype == torch.float32:
        assert err["y"] <= 4 * e32["y"] and err["dx"] <= 4 * e32["dx"], (err, e32)
        return
    # 16-bit outputs, elementwise: the fp64 result rounded to the type, to one unit in its last place -- or, where the
    # output cancels so far that its ulp is below fp32 accumulation error, to the fp32 rule (4x torch's fp32 error)
    for k, got, wants in (("y", y, ref["y"]), ("dx", [dx], [ref["dx"]])):
        for g, (a, b) in enumerate(zip(got, wants)):
            want = b.to(dtype).double()
            off = (_ulp_dist(a, want, dtype) > 1) & ((a - want).abs() > 4 * e32[k])
            assert not bool(off.any()), (k, g, int(off.sum()), (a - want).abs()[off].max().item(), e32[k])


def test_conv_refusals(dev):
    from rgbx_semantic_segmentation_amd import _lib
    C = 64
    t = torch.zeros(6, C, device=dev)
    wt = torch.zeros(C, 3, 3, C, device=dev)
    fwd = (t, wt, wt, wt, t.clone(), t.clone(), t.clone(), 1, 2, 3, C, C, 12, 24, 36, C, C, 0)
    dgr = (t, t, t, wt, wt, wt, t.clone(), 1, 2, 3, C, C, 12, 24, 36, C, C, 0)
    assert _lib.try_call("cmx_aspp_conv_fwd", *fwd) == 0 and _lib.try_call("cmx_aspp_conv_dgrad", *dgr) == 0

    def with_(args, i, v):
        a = list(args)
        a[i] = v
        return a
    off = torch.zeros(6 * C + 4, device=dev)[1:]                                    # 4 bytes past a 16-byte boundary
    for entry, ok in (("cmx_aspp_conv_fwd", fwd), ("cmx_aspp_conv_dgrad", dgr)):
        for cin, cout in ((32, 64), (64, 96), (1088, 64), (64, 0)):
            assert _lib.try_call(entry, *with_(with_(ok, 10, cin), 11, cout)) == _lib.CMX_ERR_SHAPE
        assert _lib.try_call(entry, *with_(ok, 7, 0)) == _lib.CMX_ERR_SHAPE          # B = 0
        for i in (0, 3, 6):
            assert _lib.try_call(entry, *with_(ok, i, None)) == _lib.CMX_ERR_ARG     # NULL input / weight / output
        assert _lib.try_call(entry, *with_(ok, 0, off)) == _lib.CMX_ERR_ARG          # misaligned base
        assert _lib.try_call(entry, *with_(ok, 6, off)) == _lib.CMX_ERR_ARG
        assert _lib.try_call(entry, *with_(ok, 13, 0)) == _lib.CMX_ERR_ARG           # rate 0
        assert _lib.try_call(entry, *with_(ok, 15, 62)) == _lib.CMX_ERR_ARG          # row stride below the width
        assert _lib.try_call(entry, *with_(ok, 16, 66)) == _lib.CMX_ERR_ARG          # row stride off 16 bytes
        assert _lib.try_call(entry, *with_(ok, 17, 7)) == _lib.CMX_ERR_DTYPE
    dw = torch.zeros(C * 9 * C, device=dev)
    wg = (t, t, t, t, dw, dw.clone(), dw.clone(), None, 1, 2, 3, C, C, 12, 24, 36, C, C, 0)
    assert _lib.try_call("cmx_aspp_conv_wgrad", *wg) == 0                           # one chunk: no workspace
    assert _lib.try_call("cmx_aspp_conv_wgrad", *with_(with_(wg, 9, 15), 10, 20)) == _lib.CMX_ERR_ARG   # chunks need one
    assert _lib.try_call("cmx_aspp_conv_wgrad", *with_(wg, 4, None)) == _lib.CMX_ERR_ARG
    assert _lib.try_call("cmx_aspp_conv_wgrad", *with_(wg, 3, off)) == _lib.CMX_ERR_ARG
    assert _lib.try_call("cmx_aspp_conv_wgrad", *with_(wg, 11, 32)) == _lib.CMX_ERR_SHAPE
    assert _lib.try_call("cmx_aspp_conv_wgrad", *with_(wg, 15, -1)) == _lib.CMX_ERR_ARG
    assert _lib.try_call("cmx_aspp_conv_wgrad", *with_(wg, 18, 3)) == _lib.CMX_ERR_DTYPE
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 2. the align-corners upsample + concat alone
# (B, h, w, H, W, C, Cs): dyadic ratios 1/4 and 1/8; a 1 x 1 map (broadcast, scale 0); h = 1 with H > 1; identity;
# non-integer ratios; the mit_b0 64 x 96 model shape; the mit_b2 training map
UP_CASES = [(2, 3, 5, 9, 33, 64, 48), (1, 1, 1, 4, 6, 64, 8), (1, 1, 5, 3, 17, 64, 8), (2, 4, 7, 4, 7, 64, 16),
            (1, 3, 4, 17, 23, 128, 48), (2, 2, 3, 16, 24, 256, 48), (1, 15, 20, 120, 160, 256, 48)]
UP_IDS = ["a_dyadic", "b_1x1", "c_h1", "d_identity", "e_ratio", "f_b0", "g_b2"]


@functools.lru_cache(maxsize=None)
def _up_ref(kind, case, dtype, seed=0):
    B, h, w, H, W, C, Cs = case
    g = torch.Generator().manual_seed(seed)
    if kind == "exact":
        draw = lambda *s: (torch.rand(*s, generator=g) < 0.5).double()
    else:
        draw = lambda *s: torch.randn(*s, generator=g).to(dtype).double()
    lo, skip, dcat = draw(B, C, h, w), draw(B, Cs, H, W), draw(B, C + Cs, H, W)
    res = {}
    for ft in (torch.float64, torch.float32):
        a, b = (t.detach().to(ft).clone().requires_grad_(True) for t in (lo, skip))
        cat = torch.cat([TF.interpolate(a, (H, W), mode="bilinear", align_corners=True), b], 1)
        cat.backward(dcat.to(ft))
        res[ft] = {"cat": cat.detach().double(), "dlo": a.grad.double(), "dskip": b.grad.double()}
    e32 = {k: (res[torch.float64][k] - res[torch.float32][k]).abs().max().item() for k in res[torch.float64]}
    return {"lo": lo, "skip": skip, "dcat": dcat, **res[torch.float64], "e32": e32}


def _guarded(rows, C, dtype, dev, src=None, sentinel=-777.0):
    buf = torch.full((rows + 2 * GUARD, C), sentinel, dtype=dtype, device=dev)
    if src is not None:
        buf[GUARD:GUARD + rows].copy_(src.to(dtype))
    return buf, buf[GUARD:GUARD + rows]


def _run_up(ref, case, dtype, dev):
    from rgbx_semantic_segmentation_amd import _lib
    B, h, w, H, W, C, Cs = case
    code = _lib.DTYPE_CODES[dtype]
    _, lo = _guarded(B * h * w, C, dtype, dev, _rows(ref["lo"]))
    _, skip = _guarded(B * H * W, Cs, dtype, dev, _rows(ref["skip"]))
    _, dcat = _guarded(B * H * W, C + Cs, dtype, dev, _rows(ref["dcat"]))
    outs = {"cat": _guarded(B * H * W, C + Cs, dtype, dev), "dlo": _guarded(B * h * w, C, dtype, dev),
            "dskip": _guarded(B * H * W, Cs, dtype, dev)}
    _lib.call("cmx_upcat_ac_fwd", lo, skip, outs["cat"][1], B, h, w, H, W, C, Cs, code)
    _lib.call("cmx_upcat_ac_bwd", dcat, outs["dlo"][1], outs["dskip"][1], B, h, w, H, W, C, Cs, code)
    first = outs["dlo"][0].clone()
    _lib.call("cmx_upcat_ac_bwd", dcat, outs["dlo"][1], outs["dskip"][1], B, h, w, H, W, C, Cs, code)
    torch.cuda.synchronize()
    assert torch.equal(_bits(first), _bits(outs["dlo"][0])), "the backward differs from run to run"
    for k, (buf, _) in outs.items():
        guards = torch.cat([buf[:GUARD], buf[-GUARD:]])
        assert bool((guards == -777.0).all()), f"{k}: a guard row changed"
    shapes = {"cat": (B, H, W), "dlo": (B, h, w), "dskip": (B, H, W)}
    return {k: _nchw(v.double().cpu(), shapes[k]) for k, (_, v) in outs.items()}


@pytest.mark.parametrize("dtype", DTYPES)
def test_upcat_exact(dev, dtype):
    """Case a: ratios 1/4 and 1/8, every weight a multiple of 1/32, 0/1 inputs: the forward is exact in every dtype;
    the gradient sums are exact in fp32 (below 2^10 / 32), so dlo is the fp64 result rounded once."""
    case = UP_CASES[0]
    ref = _up_ref("exact", case, torch.float64)
    assert ref["dlo"].abs().max().item() < 2 ** 10 / 32
    got = _run_up(ref, case, dtype, dev)
    assert torch.equal(got["cat"].to(dtype).double(), got["cat"]) and torch.equal(got["cat"], ref["cat"])
    for k in ("dlo", "dskip"):
        assert torch.equal(got[k], ref[k].to(dtype).double()), (k, (got[k] - ref[k]).abs().max().item())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", UP_CASES, ids=UP_IDS)
def test_upcat_random(dev, case, dtype):
    ref = _up_ref("normal", case, dtype)
    got = _run_up(ref, case, dtype, dev)
    e32 = ref["e32"]
    err = {k: (got[k] - ref[k]).abs().max().item() for k in got}
    print(f"upcat random {dtype} {case}: err {err} torch-fp32 {e32}")
    assert torch.equal(got["dskip"], ref["dskip"])                  # a copy
    B, h, w, H, W, C, Cs = case
    assert torch.equal(got["cat"][:, C:], ref["skip"])
    for k in ("cat", "dlo"):
        if dtype == torch.float32:
            assert err[k] <= 4 * e32[k], (k, err, e32)
        else:
            want = ref[k].to(dtype).double()
            off = (_ulp_dist(got[k], want, dtype) > 1) & ((got[k] - want).abs() > 4 * e32[k])
            assert not bool(off.any()), (k, int(off.sum()), (got[k] - want).abs()[off].max().item(), e32[k])


def test_upcat_refusals(dev):
    from rgbx_semantic_segmentation_amd import _lib
    lo, skip, cat = torch.zeros(6, 64, device=dev), torch.zeros(24, 8, device=dev), torch.zeros(24, 72, device=dev)
    ok = (lo, skip, cat, 1, 2, 3, 4, 6, 64, 8, 0)
    bwd = (cat, lo.clone(), skip.clone(), 1, 2, 3, 4, 6, 64, 8, 0)
    assert _lib.try_call("cmx_upcat_ac_fwd", *ok) == 0 and _lib.try_call("cmx_upcat_ac_bwd", *bwd) == 0

    def with_(args, i, v):
        a = list(args)
        a[i] = v
        return a
    off = torch.zeros(24 * 72 + 4, device=dev)[1:]
    for entry, args in (("cmx_upcat_ac_fwd", ok), ("cmx_upcat_ac_bwd", bwd)):
        for i in (0, 1, 2):
            assert _lib.try_call(entry, *with_(args, i, None)) == _lib.CMX_ERR_ARG
            assert _lib.try_call(entry, *with_(args, i, off)) == _lib.CMX_ERR_ARG
        assert _lib.try_call(entry, *with_(args, 8, 32)) == _lib.CMX_ERR_SHAPE        # C % 64
        assert _lib.try_call(entry, *with_(args, 9, 4)) == _lib.CMX_ERR_SHAPE         # Cs % 8
        assert _lib.try_call(entry, *with_(args, 4, 5)) == _lib.CMX_ERR_SHAPE         # h > H
        assert _lib.try_call(entry, *with_(args, 5, 7)) == _lib.CMX_ERR_SHAPE         # w > W
        assert _lib.try_call(entry, *with_(args, 3, 0)) == _lib.CMX_ERR_SHAPE         # B = 0
        assert _lib.try_call(entry, *with_(args, 10, 5)) == _lib.CMX_ERR_DTYPE
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 3. the head alone
B, KC = 2, 9
CH = [32, 64, 160, 256]                  # mit_b0


def relmax(a, b, scale=None):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    den = b.abs().max() if scale is None else scale.detach().double().abs().max()
    return ((a - b).abs().max() / den.clamp_min(1e-30)).item()


def rel2(a, b, scale=None):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    den = b.norm() if scale is None else scale.detach().double().norm()
    return ((a - b).norm() / den.clamp_min(1e-30)).item()


def _scale(want, n, training):
    """test_gpu_fcn_head._scale: a conv bias in front of a batch-statistics BatchNorm has a gradient of exactly zero;
    the rounding an implementation leaves there is measured against that BatchNorm bias's gradient."""
    pairs = {"grad low_level.0.bias": "grad low_level.1.bias", "grad block.0.bias": "grad block.1.bias"}
    return want[pairs[n]] if (training and n in pairs) else None


def _tensors(head, out, g1, g4, training):
    d = {"out": out, "dx1": g1, "dx4": g4}
    d.update({"grad " + n: p.grad for n, p in head.named_parameters()})
    if training:
        d.update({n: b for n, b in head.named_buffers() if "running" in n})
    return d


def _ref_run(model, feats, wout, training):
    model.train(training)
    ft = next(model.parameters()).dtype
    f = [t.detach().to(ft).clone().requires_grad_(True) for t in feats]
    out = model(f)
    (out * wout.to(ft)).sum().backward()
    return _tensors(model, out, f[0].grad, f[3].grad, training)


def cpu_case(h1, w1, h4, w4, dtype, training, seed):
    """Everything of a head case that needs no GPU: the drawn (and, in fp32, settled) restatement with its two forced
    dropout masks, its inputs, the fp64 result and the yardstick's (fp32 on the CPU, or the storage emulation)."""
    torch.manual_seed(seed)
    g = torch.Generator().manual_seed(seed + 100)
    ref32 = jitter(DeepLabV3PlusRef(CH, KC), g, dtype)
    grids = [(h1, w1), (1, 1), (1, 1), (h4, w4)]           # stages 2 and 3 are not read by this head
    feats = [torch.randn(B, c, *hw, generator=g).to(dtype).double() for c, hw in zip(CH, grids)]
    masks = ((torch.rand(B, 256, h4, w4, generator=g) < 0.5).double(), (torch.rand(B, 256, h1, w1, generator=g) < 0.9).double())
    wout = torch.randn(B, KC, h1, w1, generator=g).to(dtype).double()
    ref32.set_masks(*masks)
    if dtype == torch.float32:           # the max-abs comparison needs a draw with no ReLU input at rounding level
        settle_kinks(ref32, feats, training)
    ref = copy.deepcopy(ref32).double()
    base = copy.deepcopy(ref32) if dtype == torch.float32 else emulate_storage(copy.deepcopy(ref32), dtype)
    return ref32, feats, masks, wout, _ref_run(ref, feats, wout, training), _ref_run(base, feats, wout, training)


def _product_head(ref, dtype, dev):
    from rgbx_semantic_segmentation_amd.models.decoders.deeplabv3plus import DeepLabV3Plus
    from rgbx_semantic_segmentation_amd.params import ParamStore
    prod = DeepLabV3Plus(CH, KC)
    prod.load_state_dict(ref.state_dict(), strict=True)
    for mod in prod.modules():
        for k, buf in list(mod._buffers.items()):
            if buf is not None:
                mod._buffers[k] = buf.to(dev)
    return prod, ParamStore(prod, dev, dtype)


def _head_case(h1, w1, h4, w4, dtype, training, seed, dev):
    from rgbx_semantic_segmentation_amd import deferred
    ref32, feats, masks, wout, want, yard = cpu_case(h1, w1, h4, w4, dtype, training, seed)
    prod, store = _product_head(ref32, dtype, dev)
    prod.train(training)
    prod.forced_masks = {"dlv3_aspp_dropout": masks[0].permute(0, 2, 3, 1).to(dev),
                         "dlv3_block_dropout": masks[1].permute(0, 2, 3, 1).to(dev)} if training else None
    ft = [_rows(t).to(dtype).to(dev).requires_grad_(i in (0, 3)) for i, t in enumerate(feats)]
    out = prod.run(store, ft, [(h1, w1), (1, 1), (1, 1), (h4, w4)], B, training)
    (out * _rows(wout).to(dtype).to(dev)).sum().backward()
    deferred.flush()
    torch.cuda.synchronize()
    got = _tensors(prod, _nchw(out, (B, h1, w1)), _nchw(ft[0].grad, (B, h1, w1)), _nchw(ft[3].grad, (B, h4, w4)), training)
    assert set(got) == set(want)
    return got, want, yard


# the mit_b0 stage grids at 64 x 96 and 64 x 416 (h1, w1, h4, w4).  The seed is chosen on the CPU by the yardsticks' own
# conditions (never by a GPU result), scanning seeds 0 and 1 with cpu_case: seed 0 meets e32 < 1e-4 (after
# settle_kinks; the largest 6.6e-6) at both cases in both modes and keeps the 16-bit emulations below 0.25 everywhere
# but at (16, 24, 2, 3) in train mode, where the pooled branch's BatchNorm sees two rows and the bf16 emulation is at
# 1.02 (grad aspp.b4.gap.1.weight); seed 1 keeps both 16-bit types below 0.25 there in both modes (the largest 0.149),
# so that case's 16-bit runs take it, as test_gpu_easpp.py does for its 2 x 3 map
HEAD_SEED = 0
HEAD_SEEDS_16 = {(16, 24, 2, 3): 1}
HEAD_CASES = [(16, 24, 2, 3), (16, 104, 2, 13)]
HEAD_IDS = ["16x24_2x3", "16x104_2x13"]


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("case", HEAD_CASES, ids=HEAD_IDS)
def test_head_fp32(dev, case, training):
    got, want, yard = _head_case(*case, torch.float32, training, HEAD_SEED, dev)
    sc = {n: _scale(want, n, training) for n in want}
    rows = sorted(((relmax(got[n], want[n], sc[n]), relmax(yard[n], want[n], sc[n]), n) for n in want), reverse=True)
    print(f"head fp32 {case} train={training}: worst {rows[:3]}; largest e32 {max(r[1] for r in rows):.2e}")
    assert all(e32 < 1e-4 for _, e32, _ in rows), [r for r in rows if r[1] >= 1e-4]
    bad = [r for r in rows if r[0] > 10 * r[1]]
    assert not bad, bad[:8]


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("case", HEAD_CASES, ids=HEAD_IDS)
def test_head_16bit(dev, case, dtype, training):
    got, want, yard = _head_case(*case, dtype, training, HEAD_SEEDS_16.get(case, HEAD_SEED), dev)
    sc = {n: _scale(want, n, training) for n in want}
    rows = sorted(((rel2(got[n], want[n], sc[n]), rel2(yard[n], want[n], sc[n]), n) for n in want),
                  key=lambda r: r[0] / max(r[1], 1e-30), reverse=True)
    print(f"head {dtype} {case} train={training}: worst ratios "
          f"{[(round(r[0] / max(r[1], 1e-30), 2), r[2]) for r in rows[:3]]}; largest e_emu {max(r[1] for r in rows):.3f}")
    assert all(ee < 0.25 for _, ee, _ in rows), [r for r in rows if r[1] >= 0.25]
    bad = [r for r in rows if r[0] > 4 * r[1]]
    assert not bad, bad[:8]


# ------------------------------------------------------------------ 4. the random masks
def test_random_dropout_masks(dev):
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(1)
    h1, w1, h4, w4 = 16, 24, 2, 3
    prod, store = _product_head(jitter(DeepLabV3PlusRef(CH, KC), g), torch.float32, dev)
    for which, p, n in (("dlv3_aspp_dropout", 0.5, 1 << 18), ("dlv3_block_dropout", 0.1, 1 << 18)):
        s1 = prod.dropout_scale(which, p, n, dev).clone()
        s2 = prod.dropout_scale(which, p, n, dev).clone()
        torch.cuda.synchronize()
        keep = (torch.ones(()) / (torch.ones(()) - torch.tensor(p))).item()               # the fp32 quotient
        for s in (s1, s2):
            assert bool(((s == 0) | (s == keep)).all())
            share = (s != 0).double().mean().item()
            assert abs(share - (1 - p)) < 5 * (p * (1 - p) / n) ** 0.5, (which, share)    # 5 sigma of n draws
        differ = ((s1 != 0) != (s2 != 0)).double().mean().item()
        assert abs(differ - 2 * p * (1 - p)) < 0.02, (which, differ)                      # independent draws
        assert prod._mask_states[which][1].tolist() == [2, 0]                             # a step counter of its own
    feats = [torch.randn(B * h * w, c, generator=g).to(dev) for c, (h, w) in zip(CH, ((h1, w1), (1, 1), (1, 1), (h4, w4)))]
    grids = [(h1, w1), (1, 1), (1, 1), (h4, w4)]
    prod.train()
    with torch.no_grad():
        prod.run(store, feats, grids, B, True)                                            # eager first
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            prod.run(store, feats, grids, B, True)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            out = prod.run(store, feats, grids, B, True)
        outs = []
        for _ in range(2):
            graph.replay()
            torch.cuda.synchronize()
            outs.append(out.clone())
        assert not torch.equal(outs[0], outs[1])                                          # fresh masks on replay
        steps = {k: v[1][0].item() for k, v in prod._mask_states.items()}
        assert steps == {"dlv3_aspp_dropout": 6, "dlv3_block_dropout": 6}
        prod.eval()
        e1 = prod.run(store, feats, grids, B, False).clone()
        e2 = prod.run(store, feats, grids, B, False)
        torch.cuda.synchronize()
        assert torch.equal(e1, e2) and {k: v[1][0].item() for k, v in prod._mask_states.items()} == steps


def test_capture_before_the_first_eager_step_raises(dev):
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(1)
    prod, store = _product_head(jitter(DeepLabV3PlusRef(CH, KC), g), torch.float32, dev)
    grids = [(16, 24), (1, 1), (1, 1), (2, 3)]
    feats = [torch.randn(B * h * w, c, generator=g).to(dev) for c, (h, w) in zip(CH, grids)]
    prod.train()
    torch.cuda.synchronize()
    for which, p in (("dlv3_aspp_dropout", 0.5), ("dlv3_block_dropout", 0.1)):
        with pytest.raises(RuntimeError, match="before a graph capture"):
            with torch.cuda.graph(torch.cuda.CUDAGraph(), capture_error_mode="thread_local"):
                prod.dropout_scale(which, p, 1024, dev)        # the first draw of either dropout, inside a capture
    assert not prod.__dict__.get("_mask_states")
    with pytest.raises(ValueError, match="more than 1 image"):
        prod.run(store, [f[:f.shape[0] // 2] for f in feats], grids, 1, True)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 5. - 7. the whole model
def _pair(dtype, aux=True, criterion=None, seed=0):
    from rgbx_semantic_segmentation_amd.models.builder import EncoderDecoder
    torch.manual_seed(seed)
    ref = ref_model("mit_b0", aux_head=aux, num_classes=KC)
    g = torch.Generator().manual_seed(seed + 1)
    for n, b in ref.named_buffers():             # non-trivial BN running statistics
        if n.endswith("running_mean"):
            b.copy_(torch.rand(b.shape, generator=g) * 0.2 - 0.1)
        elif n.endswith("running_var"):
            b.copy_(torch.rand(b.shape, generator=g) + 0.5)
    cfg = dict(backbone="mit_b0", decoder="DeepLabV3Plus", num_classes=KC, compute_dtype=dtype)
    if not aux:
        cfg["aux_head"] = False
    model = EncoderDecoder(cfg, criterion=criterion).cuda()
    assert (model.aux_head is not None) == aux and set(model.state_dict()) == set(ref.state_dict())
    model.load_state_dict(ref.state_dict(), strict=True)
    return ref, model


def _batch(H=64, W=96, seed=3):
    g = torch.Generator().manual_seed(seed)
    rgb = torch.randn(B, 3, H, W, generator=g)
    x = torch.randn(B, 1, H, W, generator=g).expand(B, 3, H, W).contiguous()
    lab = torch.randint(0, KC, (B, H, W), generator=g)
    lab[:, 5:20, 7:30] = 255
    return rgb, x, lab


def _head_masks(model, refs, H, W, seed=13):
    """The same two elementwise dropout keep masks for the GPU model (NHWC) and the oracles (NCHW)."""
    g = torch.Generator().manual_seed(seed)
    ma = (torch.rand(B, H // 32, W // 32, 256, generator=g) < 0.5).float()
    mb = (torch.rand(B, H // 4, W // 4, 256, generator=g) < 0.9).float()
    model.forced_masks["dlv3_aspp_dropout"], model.forced_masks["dlv3_block_dropout"] = ma, mb
    for r in refs:
        r.decode_head.set_masks(ma.permute(0, 3, 1, 2).double(), mb.permute(0, 3, 1, 2).double())


def _settle_head(ref32, model, rgb, x, H, W):
    """Settle the ReLU kinks of the restated HEAD for this batch in train mode (deeplab_ref.settle_kinks, as the head-
    alone cases do), then hand the moved BatchNorm biases to the GPU model.  Why here and not in the other model
    tests: this head sits downstream of the whole encoder and its ASPP BatchNorms see B * h4 * w4 = 12 rows at 64 x 96,
    so ONE ReLU whose input is at fp32 rounding level (the draw of seed 0 without the auxiliary head has one at 3.7e-7,
    in aspp.project.1, found in fp64 on the CPU) changes that channel's bias gradient by a twelfth and, through the
    stage-4 map, every gradient of the encoder: not a bounded outlier.  A kink inside the encoder stays covered by the
    outlier allowance, as in tests/test_gpu_easpp.py."""
    ref32.train()
    _masks(model, [ref32], B, n_calls=1)
    _head_masks(model, [ref32], H, W)
    tmp = copy.deepcopy(ref32).double()              # the copy consumes the masks and moves its own statistics
    with torch.no_grad():
        feats = [f.detach() for f in tmp.backbone(rgb.double(), x.double())]
    settle_kinks(ref32.decode_head, feats, True, tol=1e-5)
    model.load_state_dict(ref32.state_dict(), strict=True)


@pytest.mark.parametrize("config", ["aux_96", "aux_416", "noaux_96", "noaux_416", "noaux_dice_ce_96"])
def test_model_train_step_fp32(dev, config):
    """tests/test_gpu_easpp.py::test_model_train_step_fp32's bounds: eval and train-mode logits 1e-3, loss 1e-4, every
    parameter gradient 2e-3 or 10x the fp32 oracle's own error with its bounded ReLU-kink outliers, none of them in the
    head; running statistics 1e-4."""
    aux, dice, W = config.startswith("aux"), "dice_ce" in config, int(config.rsplit("_", 1)[1])
    H = 64
    crit = (lambda: dc.make_criterion("dice_ce")) if dice else (lambda: None)
    ref32, model = _pair("float32", aux, crit())
    if dice:
        ref32.criterion = crit()
    rgb, x, lab = _batch(H, W)
    _settle_head(ref32, model, rgb, x, H, W)
    ref = copy.deepcopy(ref32).double()
    with torch.no_grad():
        for m in (ref, model):
            m.eval()
        out = model(rgb.to(dev), x.to(dev))
        assert out.shape == (B, KC, H, W) and out.dtype == torch.float32
        e_eval = relmax(out, ref(rgb.double(), x.double()))
    for m in (ref, ref32, model):
        m.train()
    _masks(model, [ref, ref32], B, n_calls=2)
    _head_masks(model, [ref, ref32], H, W)
    with torch.no_grad():
        bufs = {n: b.detach().clone() for n, b in model.named_buffers()}
        lo64 = ref.encode_decode(rgb.double(), x.double())
        lo = model.encode_decode(rgb.to(dev), x.to(dev))
        for n, b in model.named_buffers():
            b.copy_(bufs[n])
        for m in (ref, ref32):                    # the logits forward above moved their BN statistics too
            m.load_state_dict({**m.state_dict(), **{n: b.to(next(m.parameters()).dtype) if b.is_floating_point()
                                                    else b for n, b in bufs.items()}})
    e_lo = relmax(lo, lo64)
    loss64 = ref(rgb.double(), x.double(), lab)
    loss64.backward()
    ref32(rgb, x, lab).backward()
    loss = model(rgb.to(dev), x.to(dev), lab.to(dev))
    loss.backward()
    torch.cuda.synchronize()
    e_loss = abs(loss.item() - loss64.item()) / abs(loss64.item())
    p64, p32 = dict(ref.named_parameters()), dict(ref32.named_parameters())
    gmax = max(p.grad.abs().max().item() for p in ref.parameters() if p.grad is not None)
    # this head reads the stage-1 and stage-4 maps (and the auxiliary head the stage-3 map): the FFMs of the other
    # stages feed nothing, torch leaves their gradients None and their slots of the gradient buffer are never written
    fed = {0, 3} | ({2} if aux else set())
    dead = tuple(f"backbone.FFMs.{s}." for s in range(4) if s not in fed)
    rows, bad = [], []
    for n, p in model.named_parameters():
        g64 = p64[n].grad
        assert p.grad is not None, n
        if n.startswith(dead):
            assert g64 is None and p32[n].grad is None and torch.count_nonzero(p.grad).item() == 0, n
            continue
        assert g64 is not None, n
        den = max(g64.abs().max().item(), 1e-6 * gmax)
        e = (p.grad.detach().double().cpu().view_as(g64) - g64).abs().max().item() / den
        e32 = (p32[n].grad.double() - g64).abs().max().item() / den
        rows.append((e, e32, n))
        if e > max(2e-3, 10 * e32):
            bad.append((e, e32, n))
    rows.sort(reverse=True)
    heads = [r for r in rows if r[2].startswith(("decode_head.", "aux_head."))]
    print(f"model fp32 {config}: eval {e_eval:.3e} logits {e_lo:.3e} loss {e_loss:.3e}; worst grads {rows[:4]}; "
          f"worst head grads {heads[:4]}")
    assert len(heads) == 28 + 6 * aux
    assert e_eval < 1e-3 and e_lo < 1e-3 and e_loss < 1e-4, (e_eval, e_lo, e_loss)
    assert len(bad) <= max(2, len(rows) // 100) and all(b[0] < (1e-1 if "channel_proj" in b[2] else 5e-2)
                                                        for b in bad), bad[:8]
    assert not [b for b in bad if b in heads], bad
    b64 = dict(ref.named_buffers())
    for n, b in model.named_buffers():
        if "running" in n:
            assert relmax(b, b64[n]) < 1e-4, n


def test_captured_step_bit_equal_to_eager(dev):
    """One bf16 training step with the aux head (forward, two losses, backward; forced masks) captured in a HIP graph
    and replayed twice: the loss and the flat gradient buffer equal the eager step's bits."""
    _, model = _pair("bfloat16")
    model.train()
    g = torch.Generator().manual_seed(5)
    nb = sum(model.backbone.depths)
    model.forced_masks = {"droppath": (torch.rand(nb, 2, 2 * B, generator=g) > 0.2).float().to(dev),
                          "dlv3_aspp_dropout": (torch.rand(B, 2, 3, 256, generator=g) < 0.5).float().to(dev),
                          "dlv3_block_dropout": (torch.rand(B, 16, 24, 256, generator=g) < 0.9).float().to(dev)}
    rgb, x, lab = (t.to(dev) for t in _batch())
    seed = torch.ones((), device=dev)
    bufs = {n: b.detach().clone() for n, b in model.named_buffers()}

    def step():
        with torch.no_grad():                     # every step from the same BN running statistics
            for n, b in model.named_buffers():
                b.copy_(bufs[n])
        loss = model(rgb, x, lab)
        loss.backward(seed)
        return loss

    step()
    loss_e = step().detach().clone()
    grad_e = model.store.grad.clone()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(grad_e).all())
    for name in ("decode_head.aspp.b1.block.0.weight", "decode_head.block.0.weight", "aux_head.conv.0.weight"):
        assert float(model.store._param_view(grad_e, model.store.slots[name]).abs().max()) > 0, name
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    gc.collect()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        static_loss = step()
    poison = grad_e.clone()
    for slot in model.store.slots.values():
        model.store._param_view(poison, slot).fill_(float("nan"))
    dead = torch.zeros_like(grad_e, dtype=torch.bool)          # the FFM of stage 2 feeds nothing: never written
    for n, slot in model.store.slots.items():
        if n.startswith("backbone.FFMs.1."):
            model.store._param_view(dead, slot).fill_(True)
    for _ in range(2):
        model.store.grad.copy_(torch.where(dead, grad_e, poison))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static_loss.view(torch.int32), loss_e.view(torch.int32))
        assert torch.equal(model.store.grad.view(torch.int32), grad_e.view(torch.int32))


def test_train_py_end_to_end(dev, tmp_path):
    """train.py --decoder DeepLabV3Plus runs two iterations at 64 x 96 with the default auxiliary head; its checkpoint
    holds both heads and reloads strictly; a reference-format checkpoint (the restatement's state_dict) loads
    strictly."""
    from rgbx_semantic_segmentation_amd.models.builder import EncoderDecoder
    ck = str(tmp_path / "ck")
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--backbone", "mit_b0", "--decoder", "DeepLabV3Plus",
           "--height", "64", "--width", "96", "--niters-per-epoch", "2", "--nepochs", "1", "--num-classes", "9",
           "--compute-dtype", "float32", "--num-workers", "0", "--checkpoint-dir", ck]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    path = os.path.join(ck, "epoch-last.pth")
    assert os.path.exists(path), os.listdir(ck)
    sd = torch.load(path, map_location="cpu", weights_only=False)["model"]
    assert "decode_head.aspp.b2.block.0.weight" in sd and "decode_head.block.4.bias" in sd
    assert "aux_head.classifier.bias" in sd
    assert all(bool(torch.isfinite(v).all()) for v in sd.values() if v.is_floating_point())
    cfg = dict(backbone="mit_b0", decoder="DeepLabV3Plus", num_classes=9, compute_dtype="float32")
    m = EncoderDecoder(cfg).cuda()
    m.load_state_dict(sd, strict=True)
    m.eval()
    rgb, x, _ = _batch()
    with torch.no_grad():
        out = m(rgb.to(dev), x.to(dev))
    torch.cuda.synchronize()
    assert out.shape == (B, 9, 64, 96) and bool(torch.isfinite(out).all())
    torch.manual_seed(7)
    ref_path = str(tmp_path / "reference_format.pth")
    torch.save({"model": ref_model("mit_b0", num_classes=9).state_dict()}, ref_path)
    m = EncoderDecoder(cfg).cuda()
    m.load_state_dict(torch.load(ref_path, map_location="cpu", weights_only=True)["model"], strict=True)
