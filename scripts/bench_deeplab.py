"""Time the DeepLabV3+ head's own kernels and the training step that carries it, at the CMX-B2 480 x 640 bs=2 shapes
in bf16:

* conv: cmx_aspp_conv_fwd / _dgrad / _wgrad at (2, 15, 20), 512 -> 256, rates 12 / 24 / 36, HIP events around 200
  launches after 20 warm-up launches, in us per launch, with the MAC rate of the 11 live taps;
* upcat: cmx_upcat_ac_fwd / _bwd at (2, 15 x 20 -> 120 x 160, 256 + 48), in us per launch and achieved GB/s on the
  bytes the launch must move (forward: lo + skip read, cat written; backward: dcat read, dlo + dskip written);
* head: DeepLabV3Plus.run forward + backward in eager launches (weight gradients flushed) with the number of library
  launches, and the same with one part timed alone (the ASPP convolutions, block[0]'s im2col conv, the block dropout's
  scale draw), to say what dominates;
* step: the training step (bench.py's: forward, loss, backward, FusedAdamW; captured in a HIP graph and replayed) of
  mit_b2 + DeepLabV3Plus with its auxiliary head beside mit_b2 + MLPDecoder, alternating, in both orders, in ms.
Usage: python scripts/bench_deeplab.py [rounds] [conv|upcat|head|step ...]"""
import gc
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rgbx_semantic_segmentation_amd import _lib, deferred  # noqa: E402
from rgbx_semantic_segmentation_amd import functions as F  # noqa: E402
from rgbx_semantic_segmentation_amd import kernels as K  # noqa: E402
from rgbx_semantic_segmentation_amd.models.decoders.deeplabv3plus import DeepLabV3Plus  # noqa: E402
from rgbx_semantic_segmentation_amd.params import ParamStore  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
PARTS = sys.argv[2:] or ["conv", "upcat", "head", "step"]
dev = torch.device("cuda", 0)
bf = torch.bfloat16
KC = 40
B, H4, W4, H1, W1 = 2, 15, 20, 120, 160
RATES = (12, 24, 36)


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


def series(run, n=200, warm=20):
    return ", ".join(f"{timed(run, n, warm):7.1f}" for _ in range(ROUNDS))


if "conv" in PARTS:
    Cin, Cout, M = 512, 256, B * H4 * W4
    x = torch.randn(M, Cin, device=dev).to(bf)
    Ws = tuple((torch.randn(Cout, 3, 3, Cin, device=dev) * 0.02).to(bf) for _ in range(3))
    dys = tuple(torch.randn(M, Cout, device=dev).to(bf) for _ in range(3))
    Wgs = tuple(torch.empty(Cout, 3, 3, Cin, device=dev) for _ in range(3))
    live = sum((abs(ky) * r < H4) and (abs(kx) * r < W4) for r in RATES for ky in (-1, 0, 1) for kx in (-1, 0, 1))
    gmac = live * M * Cin * Cout / 1e9
    nws = _lib.query("cmx_aspp_conv_wgrad_workspace", B, H4, W4, Cin, Cout)
    print(f"aspp conv (2, 15, 20) {Cin} -> {Cout} rates {RATES}: {live} of 27 taps live, {gmac:.3f} GMAC per direction "
          f"(padding included), wgrad workspace {nws} bytes")
    for name, run in (("fwd", lambda i: K.aspp_conv_fwd(x, Ws, B, H4, W4, RATES)),
                      ("dgrad", lambda i: K.aspp_conv_dgrad(dys, Ws, B, H4, W4, RATES)),
                      ("wgrad", lambda i: K.aspp_conv_wgrad(dys, x, Wgs, B, H4, W4, RATES))):
        t = [timed(run, 200, 20) for _ in range(ROUNDS)]
        print(f"  {name:5s}: " + ", ".join(f"{v:7.1f}" for v in t) + f" us per launch; {gmac / min(t) * 1e3:.1f} TMAC/s at best")

if "upcat" in PARTS:
    C, Cs = 256, 48
    lo = torch.randn(B * H4 * W4, C, device=dev).to(bf)
    skip = torch.randn(B * H1 * W1, Cs, device=dev).to(bf)
    dcat = torch.randn(B * H1 * W1, C + Cs, device=dev).to(bf)
    fb = 2 * (lo.numel() + skip.numel() + dcat.numel())
    bb = 2 * (dcat.numel() + lo.numel() + skip.numel())
    for name, nbytes, run in (("fwd", fb, lambda i: K.upcat_ac_fwd(lo, skip, B, H4, W4, H1, W1)),
                              ("bwd", bb, lambda i: K.upcat_ac_bwd(dcat, B, H4, W4, H1, W1, C, Cs))):
        t = [timed(run, 200, 20) for _ in range(ROUNDS)]
        print(f"upcat {name} (2, 15 x 20 -> 120 x 160, {C} + {Cs}): " + ", ".join(f"{v:7.1f}" for v in t) +
              f" us per launch; {nbytes / 1e6:.1f} MB -> {nbytes / min(t) / 1e3:.0f} GB/s at best")

if "head" in PARTS:
    CH = [64, 128, 320, 512]
    torch.manual_seed(0)
    head = DeepLabV3Plus(CH, KC)
    for mod in head.modules():
        for k, b in list(mod._buffers.items()):
            if b is not None:
                mod._buffers[k] = b.to(dev)
    store = ParamStore(head, dev, bf)
    head.train()
    grids = [(H1, W1), (60, 80), (30, 40), (H4, W4)]
    feats = [torch.randn(B * h * w, c, device=dev).to(bf).requires_grad_(i in (0, 3))
             for i, (c, (h, w)) in enumerate(zip(CH, grids))]
    dout = torch.randn(B * H1 * W1, KC, device=dev).to(bf)

    def run(i):
        head.run(store, feats, grids, B, True).backward(dout)
        deferred.flush()

    print(f"head forward + backward, eager: {launches(run)} library launches; " + series(run, 30, 5) + " us")
    convs = [b.block[0] for b in (head.aspp.b1, head.aspp.b2, head.aspp.b3)]
    g3 = [torch.randn(B * H4 * W4, 256, device=dev).to(bf) for _ in range(3)]

    def run_aspp(i):
        ys = F.aspp_conv3(store, convs, feats[3], B, H4, W4)
        torch.autograd.backward(ys, g3)

    cat = torch.randn(B, H1, W1, 304, device=dev).to(bf).requires_grad_(True)
    gz = torch.randn(1, B * H1 * W1, 256, device=dev).to(bf)

    def run_block0(i):
        z, _, _ = F.conv(store, head.block[0], cat, 1, B, H1, W1, 304, 1, 1)
        z.backward(gz)
        deferred.flush()

    n = B * H1 * W1 * 256
    print("  the three ASPP convolutions, forward + both gradients: " + series(run_aspp, 50, 5) + " us")
    print(f"  block[0] (304 -> 256, im2col buffer {B * H1 * W1 * 9 * 304 * 2 / 1e6:.0f} MB), forward + backward: "
          + series(run_block0, 30, 5) + " us")
    print(f"  the block dropout's fp32 scale ({n * 4 / 1e6:.0f} MB), one draw: "
          + series(lambda i: head.dropout_scale("dlv3_block_dropout", 0.1, n, dev), 100, 10) + " us")

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
        return graph, loss, nl, (model, opt, rgb, x, lab, seed)

    new, old = "DeepLabV3Plus + aux head", "MLPDecoder"
    steps = {old: make_step(), new: make_step(decoder="DeepLabV3Plus")}
    for rep in range(ROUNDS):
        for order in ((old, new), (new, old)):
            t = {name: timed(lambda i: steps[name][0].replay(), 20, warm=5) / 1e3 for name in order}
            print(f"round {rep} captured step, {order[0]} first: " + ", ".join(f"{n} {t[n]:.3f} ms" for n in sorted(t)))
    for name, (_, loss, nl, _) in steps.items():
        print(f"{name}: {nl} library launches per eager step (C-ABI calls seen by _lib.observer); loss after the "
              f"replays {loss.item():.4f}")
