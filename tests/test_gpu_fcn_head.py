"""FCNHead on the GPU: the module alone and the model that carries it as decode head and / or auxiliary head.

1. The head alone (models.decoders.fcnhead.FCNHead.run) against the fp64 restatement tests/fcn_ref.py, train and
   eval mode: output, dX, every parameter gradient, the running statistics, by the method and margins of
   tests/test_gpu_easpp.py::test_neck_fp32 / test_neck_16bit.  fp32: ReLU kinks settled on the CPU first
   (easpp_ref.settle_kinks), max-abs relative error per tensor <= 10 e32, e32 = the restatement in fp32 on the CPU,
   after asserting e32 < 1e-4.  16-bit: relative L2 per tensor <= 4 e_emu, e_emu = oracle.bf16_emul.emulate_storage
   of the restatement, after asserting e_emu < 0.25.
2. The whole model (mit_b0, 64 x 96, B = 2, K = 9, fp32, forced masks) in three configurations against the fp64
   oracle carrying the restated head(s), with tests/test_gpu_easpp.py::test_model_train_step_fp32's bounds; eval
   logits (B, K, H, W) against the reference; state_dict keys equal the reference model's.
3. One bf16 training step of the aux configuration captured in a HIP graph and replayed twice: bit-equal to eager.
4. train.py --decoder FCNHead --aux-head end to end.
"""
import copy
import gc
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import loss_cases as lc  # noqa: E402
from easpp_ref import settle_kinks  # noqa: E402
from fcn_ref import FCNHeadRef, jitter, ref_model  # noqa: E402
from oracle.bf16_emul import emulate_storage  # noqa: E402
from test_config_parity import _masks  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, KC = 2, 9


def relmax(a, b, scale=None):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    den = b.abs().max() if scale is None else scale.detach().double().abs().max()
    return ((a - b).abs().max() / den.clamp_min(1e-30)).item()


def rel2(a, b, scale=None):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    den = b.norm() if scale is None else scale.detach().double().norm()
    return ((a - b).norm() / den.clamp_min(1e-30)).item()


def _scale(want, n, training):
    """The tensor whose size an error of tensor ``n`` is measured against: its own fp64 value, except for the conv
    bias in train mode.  A bias in front of a batch-statistics BatchNorm has a gradient of exactly zero (the
    BatchNorm's input gradient sums to zero over the rows of every channel), so its fp64 value is pure rounding
    (1e-17) and no scale; what an implementation leaves there is the rounding of that sum of cancelling terms, whose
    uncancelled counterpart, the same sum over the same rows, is the BatchNorm bias's gradient: that is the scale."""
    return want["grad conv.1.bias"] if (training and n == "grad conv.0.bias") else None


def _rows(t):
    """NCHW (B, C, h, w) -> token-major rows (B*h*w, C)."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _nchw(rows, shape):
    b, h, w = shape
    return rows.reshape(b, h, w, -1).permute(0, 3, 1, 2)


# ------------------------------------------------------------------ 1. the head alone
def _tensors(head, out, xgrad, training):
    """{name: tensor} of everything compared: output, dX, parameter gradients, running statistics."""
    d = {"out": out, "dx": xgrad}
    d.update({"grad " + n: p.grad for n, p in head.named_parameters()})
    if training:
        d.update({n: b for n, b in head.named_buffers() if "running" in n})
    return d


def _ref_run(model, x, wout, training):
    model.train(training)
    ft = next(model.parameters()).dtype
    xi = x.detach().to(ft).clone().requires_grad_(True)
    out = model(xi)
    (out * wout.to(ft)).sum().backward()
    return _tensors(model, out, xi.grad, training)


def cpu_case(cin, h, w, b, dtype, training, seed):
    """Everything of a head case that needs no GPU: the drawn (and, in fp32, settled) restatement, its inputs, the
    fp64 result and the yardstick's (fp32 on the CPU, or the storage emulation)."""
    torch.manual_seed(seed)
    g = torch.Generator().manual_seed(seed + 100)
    ref32 = jitter(FCNHeadRef(cin, num_classes=KC), g, dtype)
    x = torch.randn(b, cin, h, w, generator=g).to(dtype).double()
    wout = torch.randn(b, KC, h, w, generator=g).to(dtype).double()
    if dtype == torch.float32:           # the max-abs comparison needs a draw with no ReLU input at rounding level
        settle_kinks(ref32, x, training)
    ref = copy.deepcopy(ref32).double()
    base = copy.deepcopy(ref32) if dtype == torch.float32 else emulate_storage(copy.deepcopy(ref32), dtype)
    return ref32, x, wout, _ref_run(ref, x, wout, training), _ref_run(base, x, wout, training)


def _head_case(cin, h, w, b, dtype, training, seed, dev):
    from rgbx_semantic_segmentation_amd import deferred
    from rgbx_semantic_segmentation_amd.models.decoders.fcnhead import FCNHead
    from rgbx_semantic_segmentation_amd.params import ParamStore
    ref32, x, wout, want, yard = cpu_case(cin, h, w, b, dtype, training, seed)
    prod = FCNHead(cin, num_classes=KC)
    prod.load_state_dict(ref32.state_dict(), strict=True)
    for mod in prod.modules():
        for k, buf in list(mod._buffers.items()):
            if buf is not None:
                mod._buffers[k] = buf.to(dev)
    store = ParamStore(prod, dev, dtype)
    prod.train(training)
    xt = _rows(x).to(dtype).to(dev).requires_grad_(True)
    out = prod.run(store, xt, b, h, w, training)
    (out * _rows(wout).to(dtype).to(dev)).sum().backward()
    deferred.flush()
    torch.cuda.synchronize()
    got = _tensors(prod, _nchw(out, (b, h, w)), _nchw(xt.grad, (b, h, w)), training)
    assert set(got) == set(want)
    return got, want, yard


# (Cin, h, w, B): 160 is no multiple of 64 (the im2col conv in every dtype), hidden 40, a BatchNorm over 12 rows;
# 256 at the same map (the implicit conv, the one-launch BatchNorm); 320 (hidden 80); 512 at the stage-4 map of the
# 480 x 640 training shape.  The seed is chosen on the CPU by the yardsticks' own conditions (never by a GPU result):
# scanning seeds 0 .. 5 with cpu_case, every one of them meets e32 < 1e-4 (after settle_kinks; the largest 1.0e-6) and
# keeps the bf16 and fp16 emulations below 0.25 (the largest 0.030) at every case in both modes, so the first is taken.
HEAD_SEED = 0
HEAD_CASES = [(160, 2, 3, 2), (256, 2, 3, 2), (320, 4, 6, 2), (512, 15, 20, 2)]
HEAD_IDS = ["160_2x3", "256_2x3", "320_4x6", "512_15x20"]


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
    got, want, yard = _head_case(*case, dtype, training, HEAD_SEED, dev)
    sc = {n: _scale(want, n, training) for n in want}
    rows = sorted(((rel2(got[n], want[n], sc[n]), rel2(yard[n], want[n], sc[n]), n) for n in want),
                  key=lambda r: r[0] / max(r[1], 1e-30), reverse=True)
    print(f"head {dtype} {case} train={training}: worst ratios "
          f"{[(round(r[0] / max(r[1], 1e-30), 2), r[2]) for r in rows[:3]]}; largest e_emu {max(r[1] for r in rows):.3f}")
    assert all(ee < 0.25 for _, ee, _ in rows), [r for r in rows if r[1] >= 0.25]
    bad = [r for r in rows if r[0] > 4 * r[1]]
    assert not bad, bad[:8]


# ------------------------------------------------------------------ 2. - 4. the whole model
CONFIGS = {"fcn": dict(decoder="FCNHead"),
           "mlp_aux": dict(decoder="MLPDecoder", aux_head=True),
           "fcn_aux_focal": dict(decoder="FCNHead", aux_head=True)}


def cfg_fcn(name):
    return CONFIGS[name]["decoder"] == "FCNHead"


def _criterion(name):
    return lc.make_criterion("focal_g4", KC) if name == "fcn_aux_focal" else None


def _pair(name, dtype, seed=0):
    from rgbx_semantic_segmentation_amd.models.builder import EncoderDecoder
    cfg = CONFIGS[name]
    torch.manual_seed(seed)
    ref = ref_model("mit_b0", fcn_decoder=cfg_fcn(name), aux_head=cfg.get("aux_head", False),
                    num_classes=KC)
    if _criterion(name) is not None:
        ref.criterion = lc.Restated(_criterion(name))
    g = torch.Generator().manual_seed(seed + 1)
    for n, b in ref.named_buffers():             # non-trivial BN running statistics
        if n.endswith("running_mean"):
            b.copy_(torch.rand(b.shape, generator=g) * 0.2 - 0.1)
        elif n.endswith("running_var"):
            b.copy_(torch.rand(b.shape, generator=g) + 0.5)
    model = EncoderDecoder(dict(backbone="mit_b0", num_classes=KC, compute_dtype=dtype, decoder_embed_dim=512, **cfg),
                           criterion=_criterion(name)).cuda()
    assert set(model.state_dict()) == set(ref.state_dict())
    model.load_state_dict(ref.state_dict(), strict=True)
    return ref, model


def _batch(H=64, W=96, seed=3):
    g = torch.Generator().manual_seed(seed)
    rgb = torch.randn(B, 3, H, W, generator=g)
    x = torch.randn(B, 1, H, W, generator=g).expand(B, 3, H, W).contiguous()
    lab = torch.randint(0, KC, (B, H, W), generator=g)
    lab[:, 5:20, 7:30] = 255
    return rgb, x, lab


@pytest.mark.parametrize("name", list(CONFIGS))
def test_model_train_step_fp32(dev, name):
    """tests/test_gpu_easpp.py::test_model_train_step_fp32's bounds: eval and train-mode logits 1e-3, loss 1e-4, every
    parameter gradient 2e-3 or 10x the fp32 oracle's own error with its bounded ReLU-kink outliers, running statistics
    1e-4."""
    H, W = 64, 96
    ref32, model = _pair(name, "float32")
    ref = copy.deepcopy(ref32).double()
    rgb, x, lab = _batch(H, W)
    with torch.no_grad():
        for m in (ref, model):
            m.eval()
        out = model(rgb.to(dev), x.to(dev))
        assert out.shape == (B, KC, H, W) and out.dtype == torch.float32
        e_eval = relmax(out, ref(rgb.double(), x.double()))
    for m in (ref, ref32, model):
        m.train()
    _masks(model, [ref, ref32], B, n_calls=2)
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
    # a configuration without the all-MLP decoder reads the stage-4 map (and the stage-3 map with the auxiliary head)
    # only: the FFMs of the other stages feed nothing, torch leaves their gradients None, and here their slots of the
    # flat gradient buffer are never written (zero in a fresh store)
    fed = ({3} if cfg_fcn(name) else {0, 1, 2, 3}) | ({2} if CONFIGS[name].get("aux_head") else set())
    dead = tuple(f"backbone.FFMs.{s}." for s in range(4) if s not in fed)
    rows, bad = [], []
    for n, p in model.named_parameters():
        g64 = p64[n].grad
        assert p.grad is not None, n
        if dead and n.startswith(dead):
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
    heads = [r for r in rows if "_head." in r[2] and ("conv." in r[2] or "classifier." in r[2])]
    print(f"model fp32 {name}: eval {e_eval:.3e} logits {e_lo:.3e} loss {e_loss:.3e}; worst grads {rows[:4]}; "
          f"worst FCN head grads {heads[:4]}")
    assert len(heads) == 6 * (cfg_fcn(name) + bool(CONFIGS[name].get("aux_head")))
    assert e_eval < 1e-3 and e_lo < 1e-3 and e_loss < 1e-4, (e_eval, e_lo, e_loss)
    assert len(bad) <= max(2, len(rows) // 100) and all(b[0] < (1e-1 if "channel_proj" in b[2] else 5e-2)
                                                        for b in bad), bad[:8]
    assert not [b for b in bad if b in heads], bad
    b64 = dict(ref.named_buffers())
    for n, b in model.named_buffers():
        if "running" in n:
            assert relmax(b, b64[n]) < 1e-4, n


def test_aux_head_is_not_run_without_a_label(dev):
    """label=None returns the main logits only and leaves the auxiliary head's running statistics alone, in train
    mode too (its result would be discarded); with a label the statistics move."""
    _, model = _pair("mlp_aux", "float32")
    model.train()
    rgb, x, lab = (t.to(dev) for t in _batch())
    bn = model.aux_head.conv[1]
    before = bn.running_mean.clone()
    with torch.no_grad():
        out = model(rgb, x)
        torch.cuda.synchronize()
        assert out.shape == (B, KC, 64, 96) and torch.equal(bn.running_mean, before)
        model(rgb, x, lab)
        torch.cuda.synchronize()
        assert not torch.equal(bn.running_mean, before)


def test_captured_step_bit_equal_to_eager(dev):
    """One bf16 training step of MLPDecoder + aux head (forward, two losses, backward; forced masks) captured in a HIP
    graph and replayed twice: the loss and the flat gradient buffer equal the eager step's bits."""
    _, model = _pair("mlp_aux", "bfloat16")
    model.train()
    g = torch.Generator().manual_seed(5)
    nb = sum(model.backbone.depths)
    model.forced_masks = {"droppath": (torch.rand(nb, 2, 2 * B, generator=g) > 0.2).float().to(dev),
                          "dropout2d": (torch.rand(B, model.decode_head.embed_dim, generator=g) > 0.1).float().to(dev)}
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
    aux_w = model.store._param_view(grad_e, model.store.slots["aux_head.conv.0.weight"])
    assert float(aux_w.abs().max()) > 0
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
    """train.py --decoder FCNHead --aux-head runs two iterations at 64 x 96; its checkpoint holds both heads and
    reloads strictly into a fresh model."""
    from rgbx_semantic_segmentation_amd.models.builder import EncoderDecoder
    ck = str(tmp_path / "ck")
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--backbone", "mit_b0", "--decoder", "FCNHead",
           "--aux-head", "--height", "64", "--width", "96", "--niters-per-epoch", "2", "--nepochs", "1",
           "--num-classes", "9", "--compute-dtype", "float32", "--num-workers", "0", "--checkpoint-dir", ck]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    path = os.path.join(ck, "epoch-last.pth")
    assert os.path.exists(path), os.listdir(ck)
    sd = torch.load(path, map_location="cpu", weights_only=False)["model"]
    assert "decode_head.conv.0.weight" in sd and "aux_head.classifier.bias" in sd
    assert all(bool(torch.isfinite(v).all()) for v in sd.values() if v.is_floating_point())
    m = EncoderDecoder(dict(backbone="mit_b0", decoder="FCNHead", aux_head=True, num_classes=9,
                            compute_dtype="float32")).cuda()
    m.load_state_dict(sd, strict=True)
    m.eval()
    rgb, x, _ = _batch()
    with torch.no_grad():
        out = m(rgb.to(dev), x.to(dev))
    torch.cuda.synchronize()
    assert out.shape == (B, 9, 64, 96) and bool(torch.isfinite(out).all())
