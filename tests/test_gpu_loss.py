"""The fused upsample + loss family on the GPU (cmx_upsample_loss_fwd_adj / functions.UpsampleLossF;
FocalLoss, CE_Focal, class-weighted CrossEntropyLoss, FocalLoss2d) against the fp64 restatement of
tests/loss_cases.py, with the bounds of test_gpu_kernels.py::test_upsample_ce: relative loss error
< 1e-5 (fp32) / 1e-2 (16-bit), relerr(dlogits) < 2 * TOL, TOL = 1e-4 (fp32) / 3e-2 (16-bit); the
reference of a 16-bit run takes the rounded logits.  Then the structural cases (uniform, zero-sum,
conservation, clamp, all ignored, containment, no-grad), the model against the oracle, graph replay
and train.py."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import loss_cases as lc  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
F32 = torch.float32


def run(dev, name, shape, dtype, lg, lab, grad=True):
    """The product path for one criterion: builder's plan of the criterion object -> UpsampleLossF.
    Returns (loss, dlogits or None) with dloss = 0.7."""
    from rgbx_semantic_segmentation_amd.functions import UpsampleLossF
    from rgbx_semantic_segmentation_amd.models.builder import _loss_plan
    B, h, w, K = shape
    ignore, spec, weight = _loss_plan(lc.make_criterion(name, K))
    assert spec is not None and ignore == lc.IGNORE
    weight = None if weight is None else weight.to(dev, torch.float32).contiguous()
    x = lg.to(dev, dtype).requires_grad_(grad)
    dims = (B, h, w, 4 * h, 4 * w, K)
    if not grad:
        with torch.no_grad():
            return UpsampleLossF.apply(x, lab.to(dev), dims, ignore, spec, weight), None
    loss = UpsampleLossF.apply(x, lab.to(dev), dims, ignore, spec, weight)
    (loss * lc.DLOSS).backward()
    torch.cuda.synchronize()
    return loss.detach(), x.grad


def check(name, shape, dtype, loss, dl, ref):
    le = abs(loss.item() - ref.loss.item()) / abs(ref.loss.item())
    ge = lc.relerr(dl.view_as(ref.dlogits), ref.dlogits)
    print(f"loss family {name} {shape} {dtype}: loss rel err {le:.3e}, dlogits rel err {ge:.3e}")
    assert le < lc.LOSS_TOL[dtype], (le, loss.item(), ref.loss.item())
    assert ge < 2 * lc.TOL[dtype], ge


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", lc.SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("name", list(lc.CRITERIA))
def test_loss_and_gradient(dev, name, shape, dtype):
    lg, lab = lc.make_inputs(shape)
    loss, dl = run(dev, name, shape, dtype, lg, lab)
    check(name, shape, dtype, loss, dl, lc.expected(name, shape, dtype))


def test_focal_training_shape_bf16(dev):
    """(2, 120, 160, 40): the CMX-B2 480 x 640 training shape, FocalLoss gamma 4."""
    lg, lab = lc.make_inputs(lc.BIG)
    loss, dl = run(dev, "focal_g4", lc.BIG, torch.bfloat16, lg, lab)
    check("focal_g4", lc.BIG, torch.bfloat16, loss, dl, lc.expected("focal_g4", lc.BIG, torch.bfloat16))


@pytest.mark.parametrize("name", ["focal_g0", "focal_g4"])
def test_uniform_closed_form(dev, name):
    """All-zero logits at K = 9: every p_k = 1/K, so the loss has a closed form; a padded class
    (31 of them) leaking into the class sums would move it (at gamma = 0 by log(1 + eps) each)."""
    shape = lc.SHAPES[1]
    lg, lab = lc.make_inputs(shape, kind="uniform")
    loss, dl = run(dev, name, shape, F32, lg, lab)
    n = int((lab != lc.IGNORE).sum())
    want = lc.uniform_focal_loss(shape[3], lc.CRITERIA[name][1]) * n / (n + 1e-8)
    assert abs(loss.item() - want) / want < lc.LOSS_TOL[F32], (loss.item(), want)
    check(name, shape, F32, loss, dl, lc.expected(name, shape, F32, "uniform"))


@pytest.mark.parametrize("name", list(lc.CRITERIA))
def test_zero_sum_and_conservation(dev, name):
    """Every per-pixel gradient sums to 0 over the classes and the adjoint is linear, so dlogits sums
    to 0 over k at every low-res pixel, to within the gradient bound x max|dlogits|.  A full-res
    pixel's adjoint weights sum to 1, so the sum of dlogits[..., k] over the low-res pixels equals
    the fp64 reference's sum of the full-res gradient of class k; bound: every one of the N low-res
    elements may be off by the elementwise bound 2 TOL max|ref|, added up at worst linearly."""
    shape = lc.SHAPES[2]
    B, h, w, K = shape
    lg, lab = lc.make_inputs(shape)
    _, dl = run(dev, name, shape, F32, lg, lab)
    ref = lc.expected(name, shape, F32)
    dl = dl.double().cpu().view(B, h, w, K)
    gmax = ref.dlogits.abs().max().item()
    assert dl.sum(-1).abs().max().item() <= 2 * lc.TOL[F32] * gmax
    assert (dl.sum(dim=(0, 1, 2)) - ref.gsum).abs().max().item() <= B * h * w * 2 * lc.TOL[F32] * gmax


def test_focal_clamps_out_of_range_labels(dev):
    """Under pure FocalLoss a label K + 3 (neither the ignore value nor in range) counts as class
    K - 1 and as valid: same bits as the label K - 1 there, and not the bits of an ignored pixel."""
    shape = lc.SHAPES[1]
    K = shape[3]
    lg, lab = lc.make_inputs(shape)
    res = {}
    for v in (K + 3, K - 1, lc.IGNORE):
        lab[0, 40, 33] = v
        res[v] = run(dev, "focal_g2", shape, F32, lg, lab)
    assert torch.equal(res[K + 3][0], res[K - 1][0]) and torch.equal(res[K + 3][1], res[K - 1][1])
    assert not torch.equal(res[K + 3][1], res[lc.IGNORE][1])
    lab[0, 40, 33] = K + 3
    from rgbx_semantic_segmentation_amd.utils.loss_opr import FocalLoss
    ref = lc.reference_of(FocalLoss(lc.IGNORE, gamma=2.0, alpha=lc.ALPHA), lg, lab)
    check("focal_g2 clamp", shape, F32, *res[K + 3], ref)


def test_all_ignored(dev):
    """No valid pixel: FocalLoss gives loss 0 and a zero gradient; weighted CE a NaN loss (torch's mean)."""
    shape = lc.SHAPES[2]
    lg, lab = lc.make_inputs(shape, ignored="all")
    loss, dl = run(dev, "focal_g4", shape, F32, lg, lab)
    assert loss.item() == 0.0 and torch.count_nonzero(dl).item() == 0
    loss, _ = run(dev, "wce", shape, F32, lg, lab)
    assert torch.isnan(loss).item()


@pytest.mark.parametrize("name", ["focal_g4", "ce_focal", "fl2d_w"])
def test_containment(dev, name):
    """adj and dlogits sit inside larger NaN-filled allocations with guard rows before and after:
    the kernels write exactly their (B, h, w, K) elements and the guards come back bit-equal."""
    from rgbx_semantic_segmentation_amd import kernels as Kn
    from rgbx_semantic_segmentation_amd.models.builder import _loss_plan
    shape = lc.SHAPES[2]
    B, h, w, K = shape
    H, W = 4 * h, 4 * w
    ignore, spec, weight = _loss_plan(lc.make_criterion(name, K))
    weight = None if weight is None else weight.to(dev, torch.float32).contiguous()
    lg, lab = lc.make_inputs(shape)
    x, labd = lg.to(dev, torch.bfloat16).contiguous(), lab.to(dev)
    n, guard = B * h * w * K, 3 * w * K
    adj_buf = torch.full((n + 2 * guard,), float("nan"), device=dev)
    dl_buf = torch.full((n + 2 * guard,), float("nan"), device=dev).to(torch.bfloat16)
    adj, dl = adj_buf[guard:guard + n], dl_buf[guard:guard + n]
    bits = [(buf, buf.view(it), buf.view(it).clone()) for buf, it in ((adj_buf, torch.int32), (dl_buf, torch.int16))]
    out = torch.empty(3, device=dev)
    ws = Kn._ws(Kn.query("cmx_upsample_loss_workspace", B, h, w), dev)
    Kn.call("cmx_upsample_loss_fwd_adj", Kn.ptr(x), Kn.ptr(labd), Kn.ptr(weight), adj.data_ptr(), Kn.ptr(out),
            Kn.ptr(ws), B, h, w, H, W, K, ignore, *spec, Kn.dtype_code(x), Kn.stream())
    dloss = torch.full((1,), lc.DLOSS, device=dev)
    Kn.call("cmx_upsample_ce_bwd_scale", adj.data_ptr(), Kn.ptr(dloss), Kn.ptr(out), dl.data_ptr(), n,
            Kn.dtype_code(x), Kn.stream())
    torch.cuda.synchronize()
    for buf, now, before in bits:
        assert torch.equal(now[:guard], before[:guard]) and torch.equal(now[guard + n:], before[guard + n:])
        assert torch.isfinite(buf[guard:guard + n]).all()
    check(name, shape, torch.bfloat16, out[0], dl, lc.expected(name, shape, torch.bfloat16))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", lc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_plain_ce_equals_unweighted_kind0(dev, shape, dtype):
    """cmx_upsample_ce_fwd_adj and cmx_upsample_loss_fwd_adj with kind 0 and a null weight give the
    same bits in out (all three floats) and adj: the two criteria of the one cells kernel differ only
    by multiplications with 1.0f and additions of +0.0f."""
    from rgbx_semantic_segmentation_amd import kernels as Kn
    from rgbx_semantic_segmentation_amd.functions import LOSS_WCE
    B, h, w, K = shape
    H, W = 4 * h, 4 * w
    lg, lab = lc.make_inputs(shape)
    x, labd = lg.to(dev, dtype).contiguous(), lab.to(dev)
    adj = [torch.full((B, h, w, K), float("nan"), device=dev) for _ in range(2)]
    out = [torch.full((3,), float("nan"), device=dev) for _ in range(2)]
    ws = Kn._ws(max(Kn.query("cmx_upsample_ce_workspace", B, H, W), Kn.query("cmx_upsample_loss_workspace", B, h, w)),
                dev)
    Kn.call("cmx_upsample_ce_fwd_adj", Kn.ptr(x), Kn.ptr(labd), Kn.ptr(adj[0]), Kn.ptr(out[0]), Kn.ptr(ws), B, h, w,
            H, W, K, lc.IGNORE, Kn.dtype_code(x), Kn.stream())
    Kn.call("cmx_upsample_loss_fwd_adj", Kn.ptr(x), Kn.ptr(labd), 0, Kn.ptr(adj[1]), Kn.ptr(out[1]), Kn.ptr(ws), B,
            h, w, H, W, K, lc.IGNORE, LOSS_WCE, 0.0, 0.0, 0.0, 0.0, Kn.dtype_code(x), Kn.stream())
    torch.cuda.synchronize()
    assert torch.isfinite(out[0]).all() and torch.isfinite(adj[0]).all()
    assert torch.equal(out[0], out[1]), (out[0].tolist(), out[1].tolist())
    assert torch.equal(adj[0], adj[1]), float((adj[0] - adj[1]).abs().max())


def test_containment_plain_ce(dev):
    """The plain-CE entry points at SHAPES[2] in bf16: cmx_upsample_ce_fwd_adj's fp32 adj and
    cmx_upsample_ce_bwd's bf16 dlogits (the recompute backward's store in the logits' dtype) each sit
    inside a NaN-filled allocation with guard rows, which come back bit-equal around a finite interior."""
    from rgbx_semantic_segmentation_amd import kernels as Kn
    shape = lc.SHAPES[2]
    B, h, w, K = shape
    H, W = 4 * h, 4 * w
    lg, lab = lc.make_inputs(shape)
    x, labd = lg.to(dev, torch.bfloat16).contiguous(), lab.to(dev)
    n, guard = B * h * w * K, 3 * w * K
    adj_buf = torch.full((n + 2 * guard,), float("nan"), device=dev)
    dl_buf = torch.full((n + 2 * guard,), float("nan"), device=dev).to(torch.bfloat16)
    adj, dl = adj_buf[guard:guard + n], dl_buf[guard:guard + n]
    bits = [(buf, buf.view(it), buf.view(it).clone()) for buf, it in ((adj_buf, torch.int32), (dl_buf, torch.int16))]
    out = torch.empty(3, device=dev)
    ws = Kn._ws(Kn.query("cmx_upsample_ce_workspace", B, H, W), dev)
    Kn.call("cmx_upsample_ce_fwd_adj", Kn.ptr(x), Kn.ptr(labd), adj.data_ptr(), Kn.ptr(out), Kn.ptr(ws), B, h, w, H,
            W, K, lc.IGNORE, Kn.dtype_code(x), Kn.stream())
    dloss = torch.full((1,), lc.DLOSS, device=dev)
    Kn.call("cmx_upsample_ce_bwd", Kn.ptr(x), Kn.ptr(labd), Kn.ptr(dloss), Kn.ptr(out), dl.data_ptr(), B, h, w, H, W,
            K, lc.IGNORE, Kn.dtype_code(x), Kn.stream())
    torch.cuda.synchronize()
    for buf, now, before in bits:
        assert torch.equal(now[:guard], before[:guard]) and torch.equal(now[guard + n:], before[guard + n:])
        assert torch.isfinite(buf[guard:guard + n]).all()
    # the recompute backward is the scaled adjoint, rounded once to bf16
    want = adj * (lc.DLOSS * out[1])
    assert lc.relerr(dl.float(), want) < 2 * lc.TOL[torch.bfloat16]


@pytest.mark.parametrize("name", list(lc.CRITERIA))
def test_no_grad_loss_is_the_training_loss(dev, name):
    """Validation (torch.no_grad()) runs the same kernel: the loss equals the training forward's bit for bit."""
    shape = lc.SHAPES[2]
    lg, lab = lc.make_inputs(shape)
    a, _ = run(dev, name, shape, torch.bfloat16, lg, lab)
    b, none = run(dev, name, shape, torch.bfloat16, lg, lab, grad=False)
    assert none is None and not b.requires_grad and torch.equal(a, b)


def test_shape_envelope_raises(dev):
    """Outside H = 4h, W = 4w, K <= 40 the family has no materialised path: NotImplementedError."""
    from rgbx_semantic_segmentation_amd.functions import LOSS_FOCAL, UpsampleLossF
    x = torch.zeros(1, 4, 4, 9, device=dev)
    lab = torch.zeros(1, 16, 18, dtype=torch.int64, device=dev)
    with pytest.raises(NotImplementedError, match="4x4 -> 16x18"):
        UpsampleLossF.apply(x, lab, (1, 4, 4, 16, 18, 9), 255, (LOSS_FOCAL, 4.0, 0.25, 0.0, 1.0), None)


# ------------------------------------------------------------------------------ model level
def _model(dev, criterion, dtype, K=9, embed=512):
    from rgbx_semantic_segmentation_amd.models.builder import EncoderDecoder
    cfg = dict(backbone="mit_b0", num_classes=K, compute_dtype=dtype, decoder_embed_dim=embed)
    return EncoderDecoder(cfg, criterion=criterion).to(dev)


def test_plain_ce_keeps_its_own_path(dev):
    """The default criterion still goes through UpsampleCEF (the benchmarked launch sequence);
    the family goes through UpsampleLossF."""
    g = torch.Generator().manual_seed(3)
    rgb, x = torch.randn(1, 3, 64, 96, generator=g).to(dev), torch.randn(1, 3, 64, 96, generator=g).to(dev)
    lab = torch.randint(0, 9, (1, 64, 96), generator=g).to(dev)
    for crit, node in ((None, "UpsampleCEFBackward"), (lc.make_criterion("ce_focal", 9), "UpsampleLossFBackward"),
                       (lc.make_criterion("wce", 9), "UpsampleLossFBackward")):
        m = _model(dev, crit, "bfloat16", embed=256)
        m.eval()
        loss = m(rgb, x, lab)
        assert type(loss.grad_fn).__name__ == node, (crit, loss.grad_fn)
        assert torch.isfinite(loss).item()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("name", ["focal_g4", "ce_focal"])
def test_model_train_step_against_oracle_fp32(dev, name):
    """mit_b0 128 x 160, K = 9, B = 2, fp32, injected masks: loss and every parameter gradient against
    oracle.cmx_ref.EncoderDecoder (fp64) with its criterion set to the restatement, by the acceptance
    rule of test_model_parity.py::test_train_step_grads_fp32: loss within 1e-4; per-parameter error
    <= max(2e-3, 10 x the plain-fp32 oracle's), the same outlier allowance."""
    from oracle.cmx_ref import EncoderDecoder as RefModel, CMXConfig
    from test_model_parity import _inject, inputs
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    K, B = 9, 2
    torch.manual_seed(0)
    ref = RefModel(CMXConfig(backbone="mit_b0", num_classes=K))
    g = torch.Generator().manual_seed(1)
    for n, b in ref.named_buffers():
        if n.endswith("running_mean"):
            b.copy_(torch.rand(b.shape, generator=g) * 0.2 - 0.1)
        elif n.endswith("running_var"):
            b.copy_(torch.rand(b.shape, generator=g) + 0.5)
    model = _model(dev, lc.make_criterion(name, K), "float32")
    sd = ref.state_dict()
    model.load_state_dict(sd, strict=True)
    ref32 = RefModel(CMXConfig(backbone="mit_b0", num_classes=K))
    ref32.load_state_dict(sd)
    ref = ref.double()
    ref.criterion = lc.Restated(lc.make_criterion(name, K))
    ref32.criterion = lc.Restated(lc.make_criterion(name, K))
    ref.train(); model.train(); ref32.train()
    rgb, x, lab = inputs(B, 128, 160, K)
    _inject(ref, model, B)
    model.forced_masks = None
    _inject(ref32, model, B)
    loss_ref = ref(rgb.double(), x.double(), lab)
    loss_ref.backward()
    ref32(rgb, x, lab).backward()
    loss = model(rgb.to(dev), x.to(dev), lab.to(dev))
    loss.backward()
    torch.cuda.synchronize()
    assert abs(loss.item() - loss_ref.item()) / abs(loss_ref.item()) < 1e-4, (loss.item(), loss_ref.item())
    ref_params, r32 = dict(ref.named_parameters()), dict(ref32.named_parameters())
    gmax = max(p.grad.abs().max().item() for p in ref.parameters())
    bad, worst = [], []
    for n, p in model.named_parameters():
        gr = ref_params[n].grad
        assert gr is not None, n
        den = max(gr.abs().max().item(), 1e-6 * gmax)
        e = (p.grad.detach().double().cpu() - gr).abs().max().item() / den
        e32 = (r32[n].grad.double() - gr).abs().max().item() / den
        worst.append((e, e32, n))
        if e > max(2e-3, 10 * e32):
            bad.append((e, e32, n, gr.abs().max().item()))
    worst.sort(reverse=True)
    print(name, "loss", loss.item(), loss_ref.item(), "worst grads (gpu err, cpu-fp32 err, name)", worst[:4])
    n_allowed = max(2, len(worst) // 100)
    assert len(bad) <= n_allowed and all(b[0] < (1e-1 if "channel_proj" in b[2] else 5e-2) for b in bad), bad[:8]


def test_graph_replay_matches_eager_ce_focal(dev):
    """The CE_Focal step (bf16, mit_b0, 96 x 128) captured in a HIP graph gives the eager run's
    gradients bit for bit: the new forward allocates nothing outside torch's allocator and never syncs."""
    from rgbx_semantic_segmentation_amd import deferred
    torch.manual_seed(0)
    model = _model(dev, lc.make_criterion("ce_focal", 9), "bfloat16", embed=256)
    model.eval()
    g = torch.Generator().manual_seed(4)
    rgb = torch.randn(2, 3, 96, 128, generator=g).to(dev)
    x = torch.randn(2, 3, 96, 128, generator=g).to(dev)
    lab = torch.randint(0, 9, (2, 96, 128), generator=g).to(dev)
    model(rgb, x, lab).backward()
    torch.cuda.synchronize()
    ref = model.store.grad.clone()
    assert torch.isfinite(ref).all() and ref.abs().max() > 0
    deferred.reserve()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        model(rgb, x, lab).backward()
    torch.cuda.current_stream().wait_stream(s)
    import gc
    gc.collect()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        model(rgb, x, lab).backward()
    model.store.grad.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(model.store.grad, ref), float((model.store.grad - ref).abs().max())


def test_train_loop_ce_focal_and_focal_amp(dev, tmp_path, monkeypatch):
    """train.py --criterion CE_Focal: a finite positive loss that a second epoch on the same samples
    lowers; --criterion FocalLoss once under --use-mixed-precision (the GradScaler path)."""
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    import train
    base = ["--backbone", "mit_b0", "--num-classes", "9", "--height", "96", "--width", "128", "--batch-size", "2",
            "--niters-per-epoch", "4", "--warm-up-epoch", "0", "--lr", "1e-4"]
    ce_focal = base + ["--criterion", "CE_Focal", "--compute-dtype", "float32", "--checkpoint-dir", str(tmp_path)]
    l1 = train.main(ce_focal + ["--nepochs", "1"])
    assert l1 == l1 and 0 < l1 < float("inf")
    l2 = train.main(ce_focal + ["--nepochs", "2", "-c", str(tmp_path / "epoch-1.pth")])
    assert l2 < l1, (l1, l2)
    l3 = train.main(base + ["--criterion", "FocalLoss", "--use-mixed-precision", "--nepochs", "1"])
    assert l3 == l3 and 0 < l3 < float("inf")
