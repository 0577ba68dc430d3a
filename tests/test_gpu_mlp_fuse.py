"""The Mix-FFN fusion of stages 1-2 (csrc/dwconv.hip: cmx_mlp_fc1_dwconv_fwd, cmx_mlp_fc2_dwconv_bwd) bit for bit
against the pair of launches each replaces, in the same process:

  forward   cmx_gemm (f0 = x W1^T + b1)  then  cmx_dwconv3x3_fwd_save   ->  f0, out, act'(z)
  backward  cmx_gemm (da = dz W2)        then  cmx_dwconv3x3_bwd_saved  ->  dh, the whole partial workspace, dW, db

No tolerance is involved: every comparison is torch.equal on the raw words.  The fused kernels compute the Linear for
their own tile + halo with the GEMM kernels' arithmetic (same MFMA, operand roles, k order and rounding points), so
any difference is a bug.  Shapes: one forward tile (8 x 16), one backward tile (16 x 16) per image with two images
per group (a halo must not read the neighbouring image), ragged on both sides for both tilings, and smaller than a
tile; C = 64 (one k tile, 4 channel blocks) and C = 128 (two k tiles, 8 channel blocks); bf16 and fp16; G = 2.

Every output sits NaN-poisoned between guard rows (tests/test_gpu_dwconv_exact.py's Guarded).  The autograd-level
test runs one stage-1 Block and the stage norm under every CMX_MLP_FUSE setting (functions.MLP_FUSE, read per call)
against setting 0: outputs, the input gradient and the whole flat gradient buffer must be equal."""
import pytest
import torch

from test_gpu_dwconv_exact import Guarded

pytestmark = pytest.mark.gpu

G = 2
SHAPES = [(1, 8, 16), (2, 16, 16), (1, 17, 19), (1, 5, 7)]          # (imgs_per_group, H, W)
WIDTHS = [(64, 256), (128, 512)]                                    # (C, hidden)
DTYPES = [torch.bfloat16, torch.float16]


def words(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same(a, b):
    return torch.equal(words(a), words(b))


def make_inputs(dtype, ipg, H, W, C, hidden, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + 7 * H + W + C)
    M = ipg * H * W
    rn = lambda *s: torch.randn(*s, generator=g)
    d = dict(x=rn(G, M, C).to(dtype), W1=(rn(G, hidden, C) * C ** -0.5).to(dtype), b1=rn(G, hidden) * 0.1,
             w=rn(G, hidden, 9) * 0.3, b=rn(G, hidden) * 0.1, dz=rn(G, M, C).to(dtype),
             W2=(rn(G, C, hidden) * hidden ** -0.5).to(dtype))
    return {k: v.cuda() for k, v in d.items()}


def forward_pair(d, ipg, H, W, C, hidden):
    """({f0, out, gprime} unfused, the same fused), each a Guarded."""
    from rgbx_semantic_segmentation_amd import kernels as Kn
    NI, M = G * ipg, ipg * H * W
    like = torch.empty(NI, H * W, hidden, dtype=d["x"].dtype)
    code = Kn.dtype_code(d["x"])
    un = {k: Guarded(like, W) for k in ("f0", "out", "gprime")}
    fu = {k: Guarded(like, W) for k in ("f0", "out", "gprime")}
    Kn.gemm(d["x"], d["W1"], un["f0"].t.view(G, M, hidden), bias=d["b1"])
    Kn.call("cmx_dwconv3x3_fwd_save", un["f0"].t, d["w"], d["b"], un["out"].t, un["gprime"].t, NI, ipg, H, W, hidden,
            Kn.ACT["gelu"], code)
    Kn.call("cmx_mlp_fc1_dwconv_fwd", d["x"], d["W1"], d["b1"], d["w"], d["b"], fu["f0"].t, fu["out"].t,
            fu["gprime"].t, NI, ipg, H, W, C, hidden, Kn.ACT["gelu"], code)
    torch.cuda.synchronize()
    return un, fu


def check_guarded(gd, what):
    for k, g in gd.items():
        assert g.guards_intact(), f"{what}: {k} was written outside its rows"
        assert torch.isfinite(g.t.float()).all(), f"{what}: {k} keeps poison (an output pixel was not written)"


@pytest.mark.parametrize("C,hidden", WIDTHS)
@pytest.mark.parametrize("ipg,H,W", SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_forward_and_backward_bitwise(dev, dtype, ipg, H, W, C, hidden):
    from rgbx_semantic_segmentation_amd import kernels as Kn
    d = make_inputs(dtype, ipg, H, W, C, hidden)
    NI, M = G * ipg, ipg * H * W
    code = Kn.dtype_code(d["x"])
    un, fu = forward_pair(d, ipg, H, W, C, hidden)
    check_guarded(un, "unfused forward")
    check_guarded(fu, "fused forward")
    for k in ("f0", "out", "gprime"):
        assert same(un[k].t, fu[k].t), (
            f"forward {k}: {(words(un[k].t) != words(fu[k].t)).sum().item()} of {un[k].t.numel()} words differ")

    # backward: h = f0 and act'(z) of the forward above; da exists only on the unfused side
    f0, gp = un["f0"].t, un["gprime"].t
    nws = Kn.query("cmx_dwconv3x3_bwd_workspace", NI, ipg, H, W, hidden) // 4
    P = Kn.query("cmx_dwconv3x3_bwd_saved_tiles", ipg, H, W)
    res = {}
    for side in ("unfused", "fused"):
        for fold in (False, True):          # partials left for a deferred reduce / folded into dW, db now
            dh = Guarded(f0, W)
            ws = torch.zeros(nws, dtype=torch.float32, device="cuda")
            dw = torch.full((G, hidden, 9), float("nan"), device="cuda") if fold else None
            db = torch.full((G, hidden), float("nan"), device="cuda") if fold else None
            if side == "unfused":
                da = torch.empty(G, M, hidden, dtype=dtype, device="cuda")
                Kn.gemm(d["dz"], d["W2"].transpose(1, 2), da)
                Kn.call("cmx_dwconv3x3_bwd_saved", da, f0, gp, d["w"], dh.t, dw, db, ws, NI, ipg, H, W, hidden, 0, code)
            else:
                Kn.call("cmx_mlp_fc2_dwconv_bwd", d["dz"], d["W2"], f0, gp, d["w"], dh.t, dw, db, ws, NI, ipg, H, W, C,
                        hidden, 0, code)
            torch.cuda.synchronize()
            check_guarded({"dh": dh}, f"{side} backward")
            res[side, fold] = (dh.t, ws, dw, db)
    for fold in (False, True):
        (dh_u, ws_u, dw_u, db_u), (dh_f, ws_f, dw_f, db_f) = res["unfused", fold], res["fused", fold]
        assert same(dh_u, dh_f), f"dh: {(words(dh_u) != words(dh_f)).sum().item()} of {dh_u.numel()} words differ"
        assert same(ws_u, ws_f), "the partial workspace differs"
        assert torch.isfinite(ws_f[:G * P * hidden * 10]).all()
        if fold:
            assert same(dw_u, dw_f) and same(db_u, db_f), "dW / db differ"


@pytest.mark.parametrize("C,hidden", WIDTHS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_halo_outside_the_image_is_zero_not_bias(dev, dtype, C, hidden):
    """x = 0 and b1 = 1 make f0 = 1 at every pixel of the image; with unit taps and no conv bias z counts the
    in-image neighbours (4 at a corner, 6 on an edge, 9 inside).  A halo that held b1 outside the image would
    give 9 everywhere."""
    ipg, H, W = 1, 17, 19
    d = make_inputs(dtype, ipg, H, W, C, hidden)
    d["x"].zero_()
    d["b1"].fill_(1.0)
    d["w"].fill_(1.0)
    d["b"].zero_()
    un, fu = forward_pair(d, ipg, H, W, C, hidden)
    assert same(fu["f0"].t, torch.ones_like(fu["f0"].t)), "f0 inside the image must be b1"
    out = fu["out"].t.view(G * ipg, H, W, hidden).float()
    corner, edge, inner = out[:, 0, 0], out[:, 0, W // 2], out[:, H // 2, W // 2]
    for name, px in (("corner", corner), ("edge", edge), ("inner", inner)):
        assert (px == px.flatten()[0]).all(), f"{name} pixels differ between channels"
    assert corner.flatten()[0] < edge.flatten()[0] < inner.flatten()[0], (
        "an out-of-image halo value of f0 acted as b1, not as the conv's zero padding: "
        f"gelu(z) at corner / edge / inner = {corner.flatten()[0]}, {edge.flatten()[0]}, {inner.flatten()[0]}")
    for k in ("out", "gprime"):
        assert same(un[k].t, fu[k].t), f"{k} differs from the unfused launches on the zero-padding case"
    check_guarded(fu, "fused forward (padding case)")


def _block_step(dev, fuse, monkeypatch):
    """One stage-1 Block (C = 64, 16 x 24 tokens, B = 2 per stream) and the stage norm, forward and backward, under
    functions.MLP_FUSE = fuse -> (block output, norm output, input gradient, flat gradient buffer)."""
    from rgbx_semantic_segmentation_amd import deferred
    from rgbx_semantic_segmentation_amd import functions as F
    from rgbx_semantic_segmentation_amd.models.encoders.dual_segformer import RGBXTransformer
    from rgbx_semantic_segmentation_amd.params import ParamStore
    monkeypatch.setattr(F, "MLP_FUSE", fuse)
    B, H, W, C = 2, 16, 24, 64
    torch.manual_seed(0)
    enc = RGBXTransformer([64, 128, 320, 512], [1, 1, 1, 1])
    model = torch.nn.Module()
    model.backbone = enc                    # the store pairs the streams by the model's parameter names
    store = ParamStore(model, dev, torch.bfloat16)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(G, B * H * W, C, generator=g).to(torch.bfloat16).to(dev).requires_grad_(True)
    wt = torch.randn(G, B * H * W, C, generator=g).to(torch.bfloat16).to(dev)
    s_attn = torch.tensor([1.25, 0.0, 1.25, 1.25], device=dev)          # DropPath scales per (stream, sample)
    s_mlp = torch.tensor([0.0, 1.25, 1.25, 1.25], device=dev)
    xo, prev, tail = enc.run_block(store, enc.block1[0], x, B, H, W, s_attn, s_mlp, next_norm=enc.norm1)
    y, _, _ = F.layernorm_res(store, enc.norm1, xo, G, scale=prev[0], rps=H * W, tap=prev[1], tail=tail)
    (y * wt).sum().backward()
    deferred.flush()
    torch.cuda.synchronize()
    return xo.detach().clone(), y.detach().clone(), x.grad.clone(), store.grad.clone()


@pytest.mark.parametrize("fuse", [1, 2, 3])
def test_block_autograd_matches_unfused(dev, monkeypatch, fuse):
    ref = _block_step(dev, 0, monkeypatch)
    got = _block_step(dev, fuse, monkeypatch)
    for name, a, b in zip(("block output", "stage-norm output", "input gradient", "parameter gradients"), ref, got):
        assert torch.isfinite(a.float()).all(), name
        assert same(a, b), f"CMX_MLP_FUSE={fuse}: {name} differ from the separate launches"
    assert ref[3].abs().sum() > 0
