"""Time the FCN head and its loss at the CMX-B2 480 x 640 bs=2 shapes in bf16:

* the loss, forward + backward (plain CE): functions.UpsampleScaledLossF (cmx_upsample_loss_scaled_fwd_adj + the
  scale launch) beside functions.UpsampleCEF, whose only path at these scales materialises the (B, H, W, K) gradient
  and runs two bilinear_adjoint_1d passes over it -- at S = 16, (B, h, w, K) = (2, 30, 40, 40), and at S = 32,
  (2, 15, 20, 40); the two alternate in one process, in both orders, HIP events around 100 forward + backward runs
  after 10 warm-up runs, in us per run; then the same for FocalLoss(gamma 4) and class-weighted CE, which have
  no other path to stand beside;
* the head forward + backward in eager launches (models.decoders.fcnhead.FCNHead.run, weight gradients flushed):
  the auxiliary head on the stage-3 map (320 -> 80 at 30 x 40) and the decode head on the stage-4 map (512 -> 128 at
  15 x 20), with the number of library launches;
* the training step (bench.py's: forward, loss, backward, FusedAdamW; captured in a HIP graph and replayed) of
  mit_b2 + MLPDecoder without and with the auxiliary head, alternating, in both orders, in ms per step, and of
  decoder="FCNHead", with the library launches of one eager step of each.
Usage: python scripts/bench_fcn.py [rounds] [loss|head|step ...]"""
import gc
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rgbx_semantic_segmentation_amd import _lib, deferred  # noqa: E402
from rgbx_semantic_segmentation_amd import functions as F  # noqa: E402
from rgbx_semantic_segmentation_amd.models.decoders.fcnhead import FCNHead  # noqa: E402
from rgbx_semantic_segmentation_amd.params import ParamStore  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
PARTS = sys.argv[2:] or ["loss", "head", "step"]
dev = torch.device("cuda", 0)
bf = torch.bfloat16
KC = 40


def timed(run, n, warm=10):
    for i in range(warm):
        run(i)
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for i in range(n):
        run(i)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n * 1e3


def launches(run):
    count = [0]
    run(0)
    _lib.observer = lambda name, fn, args: count.__setitem__(0, count[0] + 1)
    run(0)
    _lib.observer = None
    return count[0]


# ------------------------------------------------------------------ the loss
def loss_runs(S, B, h, w):
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(B, h, w, KC, generator=g) * 3).to(dev, bf).requires_grad_(True)
    lab = torch.randint(0, KC, (B, S * h, S * w), generator=g)
    lab[:, 5 * S // 4:30 * S // 4, 7 * S // 4:40 * S // 4] = 255
    lab = lab.to(dev)
    dims = (B, h, w, S * h, S * w, KC)
    one = torch.ones((), device=dev)
    cw = (0.5 + 0.37 * (torch.arange(KC) % 5).float()).to(dev)

    def fn(apply, *rest):
        def run(i):
            x.grad = None
            apply(x, lab, dims, 255, *rest).backward(one)
        return run

    return {"UpsampleScaledLossF CE": fn(F.UpsampleScaledLossF.apply, None, None),
            "UpsampleCEF (materialised)": fn(F.UpsampleCEF.apply),
            "UpsampleScaledLossF FocalLoss g4": fn(F.UpsampleScaledLossF.apply, (F.LOSS_FOCAL, 4.0, 0.25, 0.0, 1.0), None),
            "UpsampleScaledLossF weighted CE": fn(F.UpsampleScaledLossF.apply, (F.LOSS_WCE, 0.0, 0.0, 1.0, 0.0), cw)}


if "loss" in PARTS:
    for S, shape in ((16, (2, 30, 40)), (32, (2, 15, 20))):
        runs = loss_runs(S, *shape)
        new, old = "UpsampleScaledLossF CE", "UpsampleCEF (materialised)"
        print(f"x{S} {shape + (KC,)}: launches per forward + backward: new {launches(runs[new])}, "
              f"materialised {launches(runs[old])}")
        for rep in range(ROUNDS):
            for order in ((new, old), (old, new)):
                t = {name: timed(runs[name], 100) for name in order}
                print(f"round {rep} x{S} {order[0][:20]:20s} first: new {t[new]:7.1f} us, materialised {t[old]:7.1f} us")
        for name in ("UpsampleScaledLossF FocalLoss g4", "UpsampleScaledLossF weighted CE"):
            print(f"x{S} {name:34s}: " + ", ".join(f"{timed(runs[name], 100):7.1f}" for _ in range(ROUNDS)) + " us")

# ------------------------------------------------------------------ the head
if "head" in PARTS:
    for what, cin, h, w in (("aux head, stage 3", 320, 30, 40), ("decode head, stage 4", 512, 15, 20)):
        B = 2
        torch.manual_seed(0)
        head = FCNHead(cin, num_classes=KC)
        for mod in head.modules():
            for k, b in list(mod._buffers.items()):
                if b is not None:
                    mod._buffers[k] = b.to(dev)
        store = ParamStore(head, dev, bf)
        head.train()
        M = B * h * w
        x = torch.randn(M, cin, device=dev).to(bf).requires_grad_(True)
        dout = torch.randn(M, KC, device=dev).to(bf)

        def run(i):
            head.run(store, x, B, h, w, True).backward(dout)
            deferred.flush()

        print(f"{what} ({cin} -> {cin // 4} -> {KC} at {h} x {w}): {launches(run)} library launches per forward + "
              "backward; " + ", ".join(f"{timed(run, 50, warm=5):7.1f}" for _ in range(ROUNDS)) + " us")

# ------------------------------------------------------------------ the step
if "step" in PARTS:
    from rgbx_semantic_segmentation_amd.data import make_batch
    from rgbx_semantic_segmentation_amd.models.builder import EncoderDecoder
    from rgbx_semantic_segmentation_amd.optim import FusedAdamW

    def make_step(**extra):
        torch.manual_seed(12345)
        cfg = dict(backbone="mit_b2", num_classes=KC, compute_dtype="bfloat16", decoder_embed_dim=512, **extra)
        model = EncoderDecoder(cfg).cuda(dev)
        model.train()
        opt = FusedAdamW(model, lr=6e-5, betas=(0.9, 0.999), weight_decay=0.01)
        rgb, x, lab = make_batch(2, 480, 640, KC, seed=12345, device=dev)
        seed = torch.ones((), device=dev)

        def step():
            loss = model(rgb, x, lab)
            opt.zero_grad()
            loss.backward(seed)
            opt.step()
            return loss

        step()
        nl = launches(lambda i: step())
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
            loss = step()
        # the graph holds raw addresses of the model's, the optimizer's and the inputs' buffers: they must outlive it
        # (dropped, the next capture's empty_cache() would hand their memory back to the driver under the graph)
        return graph, loss, nl, (model, opt, rgb, x, lab, seed)

    steps = {"MLPDecoder": make_step(), "MLPDecoder + aux head": make_step(aux_head=True),
             "FCNHead": make_step(decoder="FCNHead")}
    for rep in range(ROUNDS):
        for order in (("MLPDecoder", "MLPDecoder + aux head", "FCNHead"), ("FCNHead", "MLPDecoder + aux head", "MLPDecoder")):
            t = {name: timed(lambda i: steps[name][0].replay(), 20, warm=5) / 1e3 for name in order}
            print(f"round {rep} captured step, {order[0]} first: " + ", ".join(f"{n} {t[n]:.3f} ms" for n in sorted(t))
                  + f"; aux head adds {t['MLPDecoder + aux head'] - t['MLPDecoder']:.3f} ms")
    for name, (_, loss, nl, _) in steps.items():
        print(f"{name}: {nl} library launches per eager step (C-ABI calls seen by _lib.observer; autograd's own "
              f"additions are not counted); loss after the replays {loss.item():.4f}")
