"""The eASPP neck of the mit_b*_w_ef_aspp backbones on the GPU.

1. The grouped dilated 3x3 convolution alone, through the C-ABI (cmx_easpp_conv_fwd / _dgrad / _wgrad), against
   torch.nn.functional.conv2d(dilation=r, padding=r) in fp64 on the CPU.  Exact cases (0/1 inputs, -1/0/1 weights with
   at most 28 non-zeros per (output channel, tap) and per (input channel, tap): every sum is an integer of magnitude
   <= 252) must be bit-equal in all three dtypes.  Random cases: fp32 outputs and every dW within 4x the error of
   torch's own fp32 CPU conv2d on the same (storage-rounded) inputs; a 16-bit output within one unit in the last
   place of the fp64 result rounded to that type.  On the normal draw that holds elementwise except where an output
   cancels to almost zero: its ulp is then below the rounding of ANY fp32 accumulation of 576 terms, and such an
   element is held to the fp32 rule instead (absolute error <= 4x torch's fp32 error).  The one-ulp bound with no
   such exception is asserted on a second draw on a dyadic grid (x in multiples of 1/8, w of 1/64), on which every
   partial sum is exact in fp32.  The grid's sums have up to 17 significant bits, so the store's rounding to
   8 / 11 bits is exercised, which the exact cases do not do.  Outputs sit inside larger sentinel-filled buffers
   (row stride > 64, guard rows, the branches adjacent): nothing outside the result may change.
2. The neck alone (models.encoders.dual_segformer.eASPP.run) against the fp64 restatement tests/easpp_ref.py, train
   mode with a forced dropout mask and eval mode: output, dX, every parameter gradient, the running statistics.
   fp32: max-abs relative error per tensor <= 10 e32, e32 = the restatement in fp32 on the CPU (the rule of
   tests/test_gpu_decoderpp.py), after asserting e32 < 1e-4 for every tensor.  16-bit: relative L2 per tensor
   <= 4 e_emu, e_emu = oracle.bf16_emul.emulate_storage of the restatement, after asserting e_emu < 0.25.  That
   16-bit bound is loose for the branch BatchNorms -- a deep BN + ReLU chain at 64 channels flips easily -- which is
   why the identical-input checks of item 1 and the fp32 case carry the proof.
3. The random dropout mask: kept share, scale, fresh per graph replay, none in eval mode.
4. The whole model (mit_b0_w_ef_aspp, K = 9, B = 2) at 64 x 96 and 64 x 416 (a 2 x 13 map: rate 12 reaches along x)
   in fp32 against the fp64 oracle with the restatement, with tests/test_gpu_decoderpp.py's bounds and outlier
   allowance; no neck tensor among the outliers; eval logits 1e-3.
5. One bf16 training step with forced masks captured in a HIP graph and replayed twice: bit-equal to eager.
6. train.py --backbone mit_b0_w_ef_aspp end to end; a reference-format checkpoint loads strictly.
7. bench.py --backbone mit_b0_w_ef_aspp returns its JSON line.
"""
import copy
import functools
import gc
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as TF

from easpp_ref import EASPPRef, jitter, ref_model, settle_kinks
from oracle.bf16_emul import emulate_storage
from test_config_parity import _masks

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
CW, WSZ = 64, 64 * 9 * 64
# (B, h, w), rates: rate 12 reaches both axes / 24 only x / 36 neither; centre taps only; all nine taps and every
# border with M = 70 no tile multiple; offset = size - 1 (one source row or column per tap); the training shape
CONV_SHAPES = [((2, 14, 26), (12, 24, 36)), ((1, 2, 3), (12, 24, 36)), ((2, 5, 7), (1, 2, 3)),
               ((3, 13, 25), (12, 24, 12)), ((2, 15, 20), (12, 24, 36))]
CONV_IDS = ["14x26", "2x3", "5x7_r123", "13x25_edge", "15x20"]
LDX, LDY, GUARD = 72, 80, 3


# ------------------------------------------------------------------ 1. the grouped convolution alone
def _draw(kind, shape, seed):
    """(x, w, dy) fp64 per branch: x, dy (B, 64, h, w) NCHW, w (64, 64, 3, 3)."""
    B, h, w = shape
    g = torch.Generator().manual_seed(seed)
    xs, ws, dys = [], [], []
    for _ in range(3):
        if kind == "exact":
            x = (torch.rand(B, CW, h, w, generator=g) < 0.5).double()
            dy = (torch.rand(B, CW, h, w, generator=g) < 0.5).double()
            co, ci = torch.arange(CW)[:, None, None], torch.arange(CW)[None, :, None]
            tap = torch.arange(9)[None, None, :]
            band = ((ci - co - 7 * tap) % CW) < 28              # 28 per row and per column of every tap
            wt = torch.randint(-1, 2, (CW, CW, 9), generator=g).double() * band
            assert int((wt != 0).sum(1).max()) <= 28 and int((wt != 0).sum(0).max()) <= 28
            wt = wt.view(CW, CW, 3, 3)
        elif kind == "grid":
            x = torch.randint(-8, 9, (B, CW, h, w), generator=g).double() / 8
            dy = torch.randint(-8, 9, (B, CW, h, w), generator=g).double() / 8
            wt = torch.randint(-16, 17, (CW, CW, 3, 3), generator=g).double() / 64
        else:
            x = torch.randn(B, CW, h, w, generator=g).double()
            dy = torch.randn(B, CW, h, w, generator=g).double()
            wt = torch.randn(CW, CW, 3, 3, generator=g).double() * (2.0 / (9 * CW)) ** 0.5
        xs.append(x), ws.append(wt), dys.append(dy)
    return xs, ws, dys


@functools.lru_cache(maxsize=None)
def _conv_ref(kind, shape, rates, dtype, seed=0):
    """Inputs (rounded to ``dtype``) and fp64 results; for the normal draw also torch's fp32 CPU results."""
    xs, ws, dys = _draw(kind, shape, seed)
    rnd = lambda t: t.to(dtype).double()
    xs, ws, dys = [rnd(t) for t in xs], [rnd(t) for t in ws], [rnd(t) for t in dys]
    out = {"x": xs, "w": ws, "dy": dys, "y": [], "dx": [], "dw": [], "e32": None}
    e32 = {"y": 0.0, "dx": 0.0, "dw": 0.0}
    for x, wt, dy, r in zip(xs, ws, dys, rates):
        res = {}
        for ft in (torch.float64, torch.float32):
            xi, wi = x.detach().to(ft).clone().requires_grad_(True), wt.detach().to(ft).clone().requires_grad_(True)
            y = TF.conv2d(xi, wi, dilation=r, padding=r)
            y.backward(dy.to(ft))
            res[ft] = (y.detach().double(), xi.grad.double(), wi.grad.double())
        for k, a, b in zip(("y", "dx", "dw"), res[torch.float64], res[torch.float32]):
            out[k].append(a)
            e32[k] = max(e32[k], (a - b).abs().max().item())
    out["e32"] = e32
    return out


def _rows(t):
    """NCHW (B, C, h, w) -> token-major rows (B*h*w, C)."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _nchw(rows, shape):
    B, h, w = shape
    return rows.reshape(B, h, w, -1).permute(0, 3, 1, 2)


def _padded(ts, M, ld, dtype, dev, sentinel=-777.0):
    """The three (M, 64) tensors (None: left as sentinel) inside one sentinel-filled (3, GUARD + M + GUARD, ld)
    buffer: (buffer, views)."""
    buf = torch.full((3, M + 2 * GUARD, ld), sentinel, dtype=dtype, device=dev)
    views = [buf[g, GUARD:GUARD + M, :CW] for g in range(3)]
    for v, t in zip(views, ts):
        if t is not None:
            v.copy_(t.to(dtype))
    return buf, views


def _untouched(buf, before, M):
    keep = torch.ones_like(buf, dtype=torch.bool)
    keep[:, GUARD:GUARD + M, :CW] = False
    it = {4: torch.int32, 2: torch.int16}[buf.element_size()]
    return torch.equal(buf.view(it)[keep], before.view(it)[keep])


def _run_conv(ref, shape, rates, dtype, dev):
    """fwd, dgrad, wgrad through the C-ABI on strided, guarded buffers -> (y, dx, dw) lists of fp64 CPU tensors
    (NCHW / (Cout, Cin, 3, 3)), after checking that nothing outside the results changed."""
    from rgbx_semantic_segmentation_amd import _lib
    B, h, w = shape
    M = B * h * w
    code = _lib.DTYPE_CODES[dtype]
    _, xv = _padded([_rows(t) for t in ref["x"]], M, LDX, dtype, dev)
    _, dyv = _padded([_rows(t) for t in ref["dy"]], M, LDX, dtype, dev)
    wt = [t.permute(0, 2, 3, 1).contiguous().to(dtype).to(dev) for t in ref["w"]]       # tap-major (Cout, kh, kw, Cin)
    ybuf, yv = _padded([None] * 3, M, LDY, dtype, dev)
    dxbuf, dxv = _padded([None] * 3, M, LDY, dtype, dev)
    dwbuf = torch.full((3, WSZ + 2 * 64), -777.0, dtype=torch.float32, device=dev)
    dwv = [dwbuf[g, 64:64 + WSZ] for g in range(3)]
    y0, dx0, dw0 = ybuf.clone(), dxbuf.clone(), dwbuf.clone()
    _lib.call("cmx_easpp_conv_fwd", *xv, *wt, *yv, B, h, w, CW, *rates, LDX, LDY, code)
    _lib.call("cmx_easpp_conv_dgrad", *dyv, *wt, *dxv, B, h, w, CW, *rates, LDX, LDY, code)
    nws = _lib.query("cmx_easpp_conv_wgrad_workspace", B, h, w)
    ws = torch.empty(max(1, nws // 4), dtype=torch.float32, device=dev)
    _lib.call("cmx_easpp_conv_wgrad", *dyv, *xv, *dwv, ws, B, h, w, CW, *rates, LDX, LDX, code)
    torch.cuda.synchronize()
    assert _untouched(ybuf, y0, M), "forward wrote outside its outputs"
    assert _untouched(dxbuf, dx0, M), "dgrad wrote outside its outputs"
    edge = torch.ones_like(dwbuf, dtype=torch.bool)
    edge[:, 64:64 + WSZ] = False
    assert torch.equal(dwbuf[edge], dw0[edge]), "wgrad wrote outside its outputs"
    y = [_nchw(v.double().cpu(), shape) for v in yv]
    dx = [_nchw(v.double().cpu(), shape) for v in dxv]
    dw = [v.view(CW, 3, 3, CW).permute(0, 3, 1, 2).double().cpu() for v in dwv]
    return y, dx, dw


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,rates", CONV_SHAPES, ids=CONV_IDS)
def test_conv_exact(dev, shape, rates, dtype):
    ref = _conv_ref("exact", shape, rates, torch.float64)
    assert max(t.abs().max().item() for t in ref["y"] + ref["dx"]) <= 252
    y, dx, dw = _run_conv(ref, shape, rates, dtype, dev)
    for g in range(3):
        for name, a, b in (("y", y, ref["y"]), ("dx", dx, ref["dx"]), ("dw", dw, ref["dw"])):
            assert torch.equal(a[g], b[g]), (name, g, (a[g] - b[g]).abs().max().item())


def _ulp_dist(a, b, dtype):
    """Elementwise distance of a and b (both representable in the 16-bit ``dtype``) in units in the last place."""
    def ordinal(t):
        i = t.to(dtype).view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (ordinal(a) - ordinal(b)).abs()


def _ulps(a, b, dtype):
    return _ulp_dist(a, b, dtype).max().item()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,rates", CONV_SHAPES, ids=CONV_IDS)
def test_conv_random(dev, shape, rates, dtype):
    ref = _conv_ref("normal", shape, rates, dtype)
    y, dx, dw = _run_conv(ref, shape, rates, dtype, dev)
    e32 = ref["e32"]
    err = {k: max((a - b).abs().max().item() for a, b in zip(got, ref[k])) for k, got in (("y", y), ("dx", dx), ("dw", dw))}
    print(f"conv random {dtype} {shape} {rates}: err {err} torch-fp32 {e32}")
    assert err["dw"] <= 4 * e32["dw"], (err, e32)
    if dtype == torch.float32:
        assert err["y"] <= 4 * e32["y"] and err["dx"] <= 4 * e32["dx"], (err, e32)
        return
    # 16-bit outputs of the normal draw, elementwise: the fp64 result rounded to the type, to one unit in its last
    # place -- or, where the output cancels so far that its ulp is below fp32 accumulation error, to the fp32 rule
    # (4x torch's own fp32 error): an fp32 sum within t of the truth rounds to within max(1 ulp, 2 t) of its rounding
    for k, got in (("y", y), ("dx", dx)):
        for g in range(3):
            want = ref[k][g].to(dtype).double()
            off = (_ulp_dist(got[g], want, dtype) > 1) & ((got[g] - want).abs() > 4 * e32[k])
            assert not bool(off.any()), (k, g, int(off.sum()), (got[g] - want).abs()[off].max().item(), e32[k])
    grid = _conv_ref("grid", shape, rates, torch.float64)
    y, dx, dw = _run_conv(grid, shape, rates, dtype, dev)
    ulps = {k: max(_ulps(a, b, dtype) for a, b in zip(got, grid[k])) for k, got in (("y", y), ("dx", dx))}
    print(f"conv grid {dtype} {shape} {rates}: ulps {ulps}")
    assert ulps["y"] <= 1 and ulps["dx"] <= 1, ulps
    assert all(torch.equal(a, b) for a, b in zip(dw, grid["dw"]))          # fp32 sums of the grid are exact


def test_conv_refusals(dev):
    from rgbx_semantic_segmentation_amd import _lib
    t = torch.zeros(6, CW, device=dev)
    wt = torch.zeros(CW, 3, 3, CW, device=dev)
    ok = (t, t, t, wt, wt, wt, t.clone(), t.clone(), t.clone(), 1, 2, 3, CW, 12, 24, 36, CW, CW, 0)
    assert _lib.try_call("cmx_easpp_conv_fwd", *ok) == 0

    def with_(i, v):
        a = list(ok)
        a[i] = v
        return a
    for entry in ("cmx_easpp_conv_fwd", "cmx_easpp_conv_dgrad"):
        assert _lib.try_call(entry, *with_(12, 32)) == _lib.CMX_ERR_SHAPE           # width 32
        assert _lib.try_call(entry, *with_(12, 128)) == _lib.CMX_ERR_SHAPE
        assert _lib.try_call(entry, *with_(9, 0)) == _lib.CMX_ERR_SHAPE             # B = 0
        assert _lib.try_call(entry, *with_(1, None)) == _lib.CMX_ERR_ARG            # NULL input
        assert _lib.try_call(entry, *with_(4, None)) == _lib.CMX_ERR_ARG            # NULL weight
        assert _lib.try_call(entry, *with_(8, None)) == _lib.CMX_ERR_ARG            # NULL output
        assert _lib.try_call(entry, *with_(14, 0)) == _lib.CMX_ERR_ARG              # rate 0
        assert _lib.try_call(entry, *with_(16, 62)) == _lib.CMX_ERR_ARG             # row stride below the width
        assert _lib.try_call(entry, *with_(18, 7)) == _lib.CMX_ERR_DTYPE
    dw = torch.zeros(WSZ, device=dev)
    wg = (t, t, t, t, t, t, dw, dw.clone(), dw.clone(), None, 1, 2, 3, CW, 12, 24, 36, CW, CW, 0)
    assert _lib.try_call("cmx_easpp_conv_wgrad", *wg) == 0                          # one chunk: no workspace
    a = list(wg)
    a[10:13] = 2, 15, 20                                                            # five chunks need one
    assert _lib.try_call("cmx_easpp_conv_wgrad", *a) == _lib.CMX_ERR_ARG
    a = list(wg)
    a[6] = None
    assert _lib.try_call("cmx_easpp_conv_wgrad", *a) == _lib.CMX_ERR_ARG
    a = list(wg)
    a[13] = 32
    assert _lib.try_call("cmx_easpp_conv_wgrad", *a) == _lib.CMX_ERR_SHAPE
    f = torch.zeros(4, device=dev)
    assert _lib.try_call("cmx_easpp_concat_fwd", None, t, t, t, f, t, 1, 6, 64, 0) == _lib.CMX_ERR_ARG
    assert _lib.try_call("cmx_easpp_concat_bwd", t, t, t, t, t, f, 1, 6, 32, 0) == _lib.CMX_ERR_SHAPE
    off = torch.zeros(6 * CW + 4, device=dev)[1:]                                   # 4 bytes past a 16-byte boundary
    cat = torch.zeros(6, 5 * CW, device=dev)
    assert _lib.try_call("cmx_easpp_concat_fwd", off, t, t, t, f, cat, 1, 6, 64, 0) == _lib.CMX_ERR_ARG
    assert _lib.try_call("cmx_easpp_concat_bwd", cat, t, off, t, t, f, 1, 6, 64, 0) == _lib.CMX_ERR_ARG
    assert _lib.try_call("cmx_easpp_pool_bwd", f, 1, 64, off, 1, 6, 64, 0) == _lib.CMX_ERR_ARG
    assert _lib.try_call("cmx_easpp_pool_bwd", f, 17, 4, t, 1, 6, 64, 0) == _lib.CMX_ERR_SHAPE
    assert _lib.try_call("cmx_easpp_dropout_mask", f, 4, 1.0, 1, torch.zeros(2, dtype=torch.int64, device=dev)) \
        == _lib.CMX_ERR_ARG
    assert _lib.try_call("cmx_easpp_dropout_mask", f, 4, 0.5, 1, None) == _lib.CMX_ERR_ARG
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 2. the neck alone
def relmax(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def rel2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _product_neck(ref, C4, dtype, dev):
    from rgbx_semantic_segmentation_amd.models.encoders.dual_segformer import eASPP
    from rgbx_semantic_segmentation_amd.params import ParamStore
    prod = eASPP(C4)
    prod.load_state_dict(ref.state_dict(), strict=True)
    for mod in prod.modules():
        for k, b in list(mod._buffers.items()):
            if b is not None:
                mod._buffers[k] = b.to(dev)
    return prod, ParamStore(prod, dev, dtype)


def _tensors(neck, out, xgrad, training):
    """{name: tensor} of everything compared: output, dX, parameter gradients, running statistics."""
    d = {"out": out, "dx": xgrad}
    d.update({"grad " + n: p.grad for n, p in neck.named_parameters()})
    if training:
        d.update({n: b for n, b in neck.named_buffers() if "running" in n})
    return d


def _ref_run(model, x, mask, wout, training):
    model.train(training)
    model.project[3].mask = mask
    ft = next(model.parameters()).dtype
    xi = x.detach().to(ft).clone().requires_grad_(True)
    out = model(xi)
    (out * wout.to(ft)).sum().backward()
    return _tensors(model, out, xi.grad, training)


def _neck_case(C4, h, w, B, dtype, training, seed, dev):
    from rgbx_semantic_segmentation_amd import deferred
    torch.manual_seed(seed)
    g = torch.Generator().manual_seed(seed + 100)
    ref32 = jitter(EASPPRef(C4), g, dtype)
    x = torch.randn(B, C4, h, w, generator=g).to(dtype).double()
    mask = (torch.rand(B, C4, h, w, generator=g) < 0.5).double()                  # NCHW keep flags
    wout = torch.randn(B, C4, h, w, generator=g).to(dtype).double()
    if dtype == torch.float32:           # the max-abs comparison needs a draw with no ReLU input at rounding level
        settle_kinks(ref32, x, training)
    prod, store = _product_neck(ref32, C4, dtype, dev)
    ref = copy.deepcopy(ref32).double()
    base = copy.deepcopy(ref32) if dtype == torch.float32 else emulate_storage(copy.deepcopy(ref32), dtype)
    want = _ref_run(ref, x, mask, wout, training)
    yard = _ref_run(base, x, mask, wout, training)
    prod.train(training)
    xt = _rows(x).to(dtype).to(dev).requires_grad_(True)
    out = prod.run(store, xt, B, h, w, training, mask=_rows(mask).to(dev) if training else None)
    (out * _rows(wout).to(dtype).to(dev)).sum().backward()
    deferred.flush()
    torch.cuda.synchronize()
    got = _tensors(prod, _nchw(out, (B, h, w)), _nchw(xt.grad, (B, h, w)), training)
    assert set(got) == set(want)
    return got, want, yard


# (C4, h, w, B).  The seed is chosen on the CPU by the yardsticks' own conditions below (never by a GPU result): of
# seeds 0 .. 23 only 5, 8 and 19 meet them at every case in both modes; the others draw a ReLU kink somewhere (one
# flipped element puts the fp32 restatement's own max-abs error at 1e-2 .. 6e-2) or put the bf16 emulation above 0.25.
# Meeting e32 < 1e-4 only says that the CPU's fp32 run flipped no ReLU: every draw at these sizes still has
# pre-activations below fp32 rounding (the nearest at 0.03 of the fp32 restatement's own error for seed 8 at
# (512, 14, 26)), where any other fp32 implementation may land on the other side.  The fp32 cases therefore settle
# the draw first (easpp_ref.settle_kinks: BatchNorm biases moved until no ReLU input is within 1e-4 of zero in fp64)
# At (256, 2, 3) every BatchNorm sees 12 rows (the pooled one 2) and seed 8 puts the bf16 emulation of the train
# mode at 0.64 (grad img_pooling.gap.1.weight); of seeds 0 .. 40 the seeds 0, 22, 25, 30 and 34 keep it below 0.25 in
# both 16-bit types and both modes there, so that case's 16-bit runs take the first of them
NECK_SEED = 8
NECK_SEEDS_16 = {(256, 2, 3, 2): 0}
NECK_CASES = [(256, 14, 26, 2), (512, 14, 26, 2), (256, 2, 3, 2), (256, 26, 38, 2)]
NECK_IDS = ["256_14x26", "512_14x26", "256_2x3", "256_26x38"]


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("case", NECK_CASES, ids=NECK_IDS)
def test_neck_fp32(dev, case, training):
    got, want, yard = _neck_case(*case, torch.float32, training, NECK_SEED, dev)
    rows = sorted(((relmax(got[n], want[n]), relmax(yard[n], want[n]), n) for n in want), reverse=True)
    print(f"neck fp32 {case} train={training}: worst {rows[:3]}; largest e32 {max(r[1] for r in rows):.2e}")
    assert all(e32 < 1e-4 for _, e32, _ in rows), [r for r in rows if r[1] >= 1e-4]
    bad = [r for r in rows if r[0] > 10 * r[1]]
    assert not bad, bad[:8]


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("case", NECK_CASES, ids=NECK_IDS)
def test_neck_16bit(dev, case, dtype, training):
    got, want, yard = _neck_case(*case, dtype, training, NECK_SEEDS_16.get(case, NECK_SEED), dev)
    rows = sorted(((rel2(got[n], want[n]), rel2(yard[n], want[n]), n) for n in want),
                  key=lambda r: r[0] / max(r[1], 1e-30), reverse=True)
    print(f"neck {dtype} {case} train={training}: worst ratios {[(round(r[0] / max(r[1], 1e-30), 2), r[2]) for r in rows[:3]]}; "
          f"largest e_emu {max(r[1] for r in rows):.3f}")
    assert all(ee < 0.25 for _, ee, _ in rows), [r for r in rows if r[1] >= 0.25]
    bad = [r for r in rows if r[0] > 4 * r[1]]
    assert not bad, bad[:8]


# ------------------------------------------------------------------ 3. the random mask
def test_random_dropout_mask(dev):
    from rgbx_semantic_segmentation_amd.models.encoders.dual_segformer import eASPP
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(1)
    C4, B, h, w = 512, 2, 15, 20
    M = B * h * w
    ref = jitter(EASPPRef(C4), g)
    prod, store = _product_neck(ref, C4, torch.float32, dev)
    n = M * C4
    s1 = prod.dropout_scale(n, dev).clone()
    s2 = prod.dropout_scale(n, dev).clone()
    torch.cuda.synchronize()
    for s in (s1, s2):
        assert bool(((s == 0) | (s == 2)).all())                                # kept elements scaled by exactly 2
        share = (s == 2).double().mean().item()
        assert abs(share - 0.5) < 4.5e-3, share                                 # 5 sigma of n = 307200 draws
    assert 0.45 < (s1 != s2).double().mean().item() < 0.55                      # the step advanced: independent draws
    assert prod._mask_state[1].tolist() == [2, 0]                               # two steps, arrival counter back at 0
    # one captured training forward of the neck, replayed twice: the masks differ, with no host involvement
    x = torch.randn(M, C4, generator=g).to(dev)
    prod.train()
    with torch.no_grad():
        prod.run(store, x, B, h, w, True)                                       # eager first: the state exists
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            prod.run(store, x, B, h, w, True)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            out = prod.run(store, x, B, h, w, True)
        zeros = []
        for _ in range(2):
            graph.replay()
            torch.cuda.synchronize()
            zeros.append((out == 0).clone())
        step = prod._mask_state[1][0].item()
        assert bool((zeros[0] != zeros[1]).any()) and 0.1 < (zeros[0] != zeros[1]).double().mean().item() < 0.55
        # eval: no mask is drawn (the step stays) and none applied (the output is the same every time)
        prod.eval()
        e1 = prod.run(store, x, B, h, w, False).clone()
        e2 = prod.run(store, x, B, h, w, False)
        torch.cuda.synchronize()
        assert torch.equal(e1, e2) and prod._mask_state[1][0].item() == step


# ------------------------------------------------------------------ 4. - 7. the whole model
B, KC = 2, 9


def _pair(dtype, seed=0):
    from rgbx_semantic_segmentation_amd.models.builder import EncoderDecoder
    torch.manual_seed(seed)
    ref = ref_model("mit_b0", num_classes=KC)
    g = torch.Generator().manual_seed(seed + 1)
    for n, b in ref.named_buffers():             # non-trivial BN running statistics
        if n.endswith("running_mean"):
            b.copy_(torch.rand(b.shape, generator=g) * 0.2 - 0.1)
        elif n.endswith("running_var"):
            b.copy_(torch.rand(b.shape, generator=g) + 0.5)
    model = EncoderDecoder(dict(backbone="mit_b0_w_ef_aspp", num_classes=KC, compute_dtype=dtype,
                                decoder_embed_dim=512)).cuda()
    model.load_state_dict(ref.state_dict(), strict=True)
    return ref, model


def _batch(H=64, W=96, seed=3):
    g = torch.Generator().manual_seed(seed)
    rgb = torch.randn(B, 3, H, W, generator=g)
    x = torch.randn(B, 1, H, W, generator=g).expand(B, 3, H, W).contiguous()
    lab = torch.randint(0, KC, (B, H, W), generator=g)
    lab[:, 5:20, 7:30] = 255
    return rgb, x, lab


def _neck_mask(model, refs, H, W, seed=13):
    """The same elementwise dropout keep mask for the GPU model (B, h, w, C4) and the oracles (NCHW)."""
    g = torch.Generator().manual_seed(seed)
    m = (torch.rand(B, H // 32, W // 32, model.channels[3], generator=g) < 0.5).float()
    model.forced_masks["aspp_dropout"] = m
    for r in refs:
        r.backbone.single_aspp.project[3].mask = m.permute(0, 3, 1, 2).double()


@pytest.mark.parametrize("W", [96, 416])
def test_model_train_step_fp32(dev, W):
    """tests/test_gpu_decoderpp.py::test_model_train_step_fp32's bounds: train-mode logits 1e-3, loss 1e-4, every
    parameter gradient 2e-3 or 10x the fp32 oracle's own error, its bounded ReLU-kink outliers, none of them in the
    neck; running statistics 1e-4; eval logits 1e-3."""
    H = 64
    ref32, model = _pair("float32")
    ref = copy.deepcopy(ref32).double()
    rgb, x, lab = _batch(H, W)
    with torch.no_grad():
        for m in (ref, model):
            m.eval()
        e_eval = relmax(model(rgb.to(dev), x.to(dev)), ref(rgb.double(), x.double()))
    for m in (ref, ref32, model):
        m.train()
    _masks(model, [ref, ref32], B, n_calls=2)
    _neck_mask(model, [ref, ref32], H, W)
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
    gmax = max(p.grad.abs().max().item() for p in ref.parameters())
    rows, bad = [], []
    for n, p in model.named_parameters():
        g64 = p64[n].grad
        assert g64 is not None and p.grad is not None, n
        den = max(g64.abs().max().item(), 1e-6 * gmax)
        e = (p.grad.detach().double().cpu().view_as(g64) - g64).abs().max().item() / den
        e32 = (p32[n].grad.double() - g64).abs().max().item() / den
        rows.append((e, e32, n))
        if e > max(2e-3, 10 * e32):
            bad.append((e, e32, n))
    rows.sort(reverse=True)
    neck = [r for r in rows if ".single_aspp." in r[2]]
    print(f"model fp32 W={W}: eval {e_eval:.3e} logits {e_lo:.3e} loss {e_loss:.3e}; worst grads {rows[:4]}; "
          f"worst neck grads {neck[:4]}")
    assert len(neck) == 54
    assert e_eval < 1e-3 and e_lo < 1e-3 and e_loss < 1e-4, (e_eval, e_lo, e_loss)
    assert len(bad) <= max(2, len(rows) // 100) and all(b[0] < (1e-1 if "channel_proj" in b[2] else 5e-2)
                                                        for b in bad), bad[:8]
    assert not [b for b in bad if ".single_aspp." in b[2]], bad
    b64 = dict(ref.named_buffers())
    for n, b in model.named_buffers():
        if "running" in n:
            assert relmax(b, b64[n]) < 1e-4, n


def test_captured_step_bit_equal_to_eager(dev):
    """One bf16 training step (forward, loss, backward; forced masks) captured in a HIP graph and replayed twice:
    the loss and the flat gradient buffer equal the eager step's bits."""
    _, model = _pair("bfloat16")
    model.train()
    g = torch.Generator().manual_seed(5)
    nb = sum(model.backbone.depths)
    model.forced_masks = {"droppath": (torch.rand(nb, 2, 2 * B, generator=g) > 0.2).float().to(dev),
                          "dropout2d": (torch.rand(B, model.decode_head.embed_dim, generator=g) > 0.1).float().to(dev),
                          "aspp_dropout": (torch.rand(B, 2, 3, model.channels[3], generator=g) < 0.5).float().to(dev)}
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
    assert bool(poison.isnan().any())
    for _ in range(2):
        model.store.grad.copy_(poison)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static_loss.view(torch.int32), loss_e.view(torch.int32))
        assert torch.equal(model.store.grad.view(torch.int32), grad_e.view(torch.int32))


def test_train_py_end_to_end(dev, tmp_path):
    """train.py --backbone mit_b0_w_ef_aspp runs two iterations; its checkpoint reloads into a fresh model that gives
    identical logits; a reference-format checkpoint (the restatement's state_dict) loads strictly."""
    from rgbx_semantic_segmentation_amd.models.builder import EncoderDecoder
    ck = str(tmp_path / "ck")
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--backbone", "mit_b0_w_ef_aspp", "--height", "64",
           "--width", "96", "--niters-per-epoch", "2", "--nepochs", "1", "--num-classes", "9", "--compute-dtype",
           "float32", "--num-workers", "0", "--checkpoint-dir", ck]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    path = os.path.join(ck, "epoch-last.pth")
    assert os.path.exists(path), os.listdir(ck)
    sd = torch.load(path, map_location="cpu", weights_only=False)["model"]
    assert "backbone.single_aspp.branch2.3.block.0.weight" in sd and "backbone.single_aspp.project.1.running_var" in sd
    cfg = dict(backbone="mit_b0_w_ef_aspp", num_classes=9, compute_dtype="float32", decoder_embed_dim=512)
    outs = []
    rgb, x, _ = _batch()
    for _ in range(2):
        m = EncoderDecoder(cfg).cuda()
        m.load_state_dict(sd, strict=True)
        m.eval()
        with torch.no_grad():
            outs.append(m(rgb.to(dev), x.to(dev)))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(outs[0]).all()) and torch.equal(outs[0], outs[1])
    torch.manual_seed(7)
    ref_path = str(tmp_path / "reference_format.pth")
    torch.save({"model": ref_model("mit_b0", num_classes=9).state_dict()}, ref_path)
    m = EncoderDecoder(cfg).cuda()
    m.load_state_dict(torch.load(ref_path, map_location="cpu", weights_only=True)["model"], strict=True)


def test_bench_returns_its_line(dev, monkeypatch, capsys):
    import bench
    monkeypatch.setenv("CMX_BENCH_SETTLE_S", "0")
    monkeypatch.setenv("CMX_BENCH_SETTLE_MAX_S", "0.2")
    monkeypatch.delenv("CMX_BENCH_TRACE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--backbone", "mit_b0_w_ef_aspp", "--height", "64",
                                      "--width", "96", "--batch", "2", "--classes", "9", "--steps", "3", "--warmup", "1"])
    capsys.readouterr()
    bench.main()
    lines = [json.loads(s) for s in capsys.readouterr().out.splitlines() if s.startswith("{")]
    assert len(lines) == 1
    line = lines[0]
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["dtype"] == "bf16"
    assert "mit_b0_w_ef_aspp" in line["config"]["model"]
