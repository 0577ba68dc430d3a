"""Time the UPerNet head's own kernels and the training step that carries it, at the CMX-B2 480 x 640 bs=2 shapes in
bf16:

* kernels: cmx_ppm_pool_fwd / _bwd on the (2, 15, 20, 512) stage-4 map; cmx_upcat_multi_fwd / _bwd for the PPM concat
  (512 + 4 x 512 at 15 x 20) and the FPN concat (4 x 512 at 120 x 160); cmx_up_add_fwd and its adjoint at the three
  top-down steps; cmx_conv_flip_weight for the five 3x3 weights; HIP events around 100 launches after 10 warm-up
  launches, in us per launch, with achieved GB/s on the bytes the launch must move;
* convs: the five 3x3 convs forward (cmx_conv_implicit_fwd), input gradient (flip + cmx_conv_implicit_fwd) and weight
  gradient (the deferred grouped launch, flushed), in us with the MAC rate;
* dgrad: fpn_convs[0]'s input gradient both ways (the im2col-free launch against dcols + col2im, through
  functions.CONV_DGRAD_IMPLICIT), with the buffer each allocates;
* head: UPerHead.run forward + backward in eager launches (weight gradients flushed) with the number of library launches;
* step: the training step (bench.py's: forward, loss, backward, FusedAdamW; captured in a HIP graph and replayed) of
  mit_b2 + UPerHead with its auxiliary head beside mit_b2 + MLPDecoder, alternating, in both orders, in ms.
Usage: python scripts/bench_uper.py [rounds] [kernels|convs|dgrad|head|step ...]"""
import gc
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rgbx_semantic_segmentation_amd import _lib, deferred  # noqa: E402
from rgbx_semantic_segmentation_amd import functions as F  # noqa: E402
from rgbx_semantic_segmentation_amd import kernels as K  # noqa: E402
from rgbx_semantic_segmentation_amd.models.decoders.UPernet import UPerHead  # noqa: E402
from rgbx_semantic_segmentation_amd.params import ParamStore  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
PARTS = sys.argv[2:] or ["kernels", "convs", "dgrad", "head", "step"]
dev = torch.device("cuda", 0)
bf = torch.bfloat16
KC, B, Ch = 40, 2, 512
CH = [64, 128, 320, 512]
GRIDS = [(120, 160), (60, 80), (30, 40), (15, 20)]
SCALES = (1, 2, 3, 6)


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


def report(name, run, nbytes=None, gmac=None, n=100, warm=10):
    t = [timed(run, n, warm) for _ in range(ROUNDS)]
    tail = ""
    if nbytes is not None:
        tail = f"; {nbytes / 1e6:.1f} MB -> {nbytes / min(t) / 1e3:.0f} GB/s at best"
    if gmac is not None:
        tail = f"; {gmac:.2f} GMAC -> {gmac / min(t) * 1e3:.1f} TMAC/s at best"
    print(f"  {name}: " + ", ".join(f"{v:8.1f}" for v in t) + " us" + tail, flush=True)
    return min(t)


def rows(i, c):
    h, w = GRIDS[i]
    return torch.randn(B * h * w, c, device=dev).to(bf)


def make_head():
    torch.manual_seed(0)
    head = UPerHead(CH, KC, Ch)
    for mod in head.modules():
        for k, b in list(mod._buffers.items()):
            if b is not None:
                mod._buffers[k] = b.to(dev)
    return head, ParamStore(head, dev, bf)


if "kernels" in PARTS:
    print("the head's own kernels, bf16, mit_b2 480 x 640 bs = 2:")
    (h4, w4), (h1, w1) = GRIDS[3], GRIDS[0]
    x4, R = rows(3, 512), B * K.ppm_rows(SCALES)
    dp = torch.randn(R, 512, device=dev).to(bf)
    report("ppm_pool_fwd (2, 15, 20, 512)", lambda i: K.ppm_pool_fwd(x4, B, h4, w4, SCALES), 2 * (x4.numel() + R * 512))
    report("ppm_pool_bwd, with add", lambda i: K.ppm_pool_bwd(dp, x4, B, h4, w4, SCALES), 2 * (3 * x4.numel() + R * 512))
    srcs = [torch.randn(B * s * s, Ch, device=dev).to(bf) for s in SCALES]
    pg = tuple((s, s) for s in SCALES)
    dcat = torch.randn(B * h4 * w4, 512 + 4 * Ch, device=dev).to(bf)
    nb = 2 * (x4.numel() + sum(t.numel() for t in srcs) + dcat.numel())
    report("upcat_multi_fwd, PPM concat (15 x 20, 512 + 4 x 512)", lambda i: K.upcat_multi_fwd(x4, srcs, B, h4, w4, pg), nb)
    report("upcat_multi_bwd, PPM concat, dskip handed over", lambda i: K.upcat_multi_bwd(dcat, B, h4, w4, 512, Ch, pg, False),
           2 * (dcat.numel() * 4 // 5 + sum(t.numel() for t in srcs)))
    outs = [rows(i, Ch) for i in range(4)]
    dcat = torch.randn(B * h1 * w1, 4 * Ch, device=dev).to(bf)
    nb = 2 * (sum(t.numel() for t in outs) + dcat.numel())
    report("upcat_multi_fwd, FPN concat (120 x 160, 4 x 512)", lambda i: K.upcat_multi_fwd(outs[0], outs[1:], B, h1, w1, GRIDS[1:]), nb)
    report("upcat_multi_bwd, FPN concat", lambda i: K.upcat_multi_bwd(dcat, B, h1, w1, Ch, Ch, GRIDS[1:]), nb)
    for i in (3, 2, 1):
        (h, w), (H, W) = GRIDS[i], GRIDS[i - 1]
        hi, lo = rows(i - 1, Ch), rows(i, Ch)
        report(f"up_add_fwd {h} x {w} -> {H} x {W}", lambda _: K.up_add_fwd(hi, lo, B, h, w, H, W), 2 * (2 * hi.numel() + lo.numel()))
        report("  its adjoint (upcat_multi_bwd, Cs = 0, n = 1)", lambda _: K.upcat_multi_bwd(hi, B, H, W, 0, Ch, ((h, w),), False),
               2 * (hi.numel() + lo.numel()))
    for cin in (2560, 2048, 512):
        Wt = torch.randn(1, Ch, 9 * cin, device=dev).to(bf)
        report(f"conv_flip_weight {cin} -> 512, 3 x 3", lambda i: K.conv_flip_weight(Wt, 3, 3, cin), 4 * Wt.numel())

CONVS = [("bottleneck", 3, 2560), ("fpn_convs[0]", 0, 512), ("fpn_convs[1]", 1, 512), ("fpn_convs[2]", 2, 512),
         ("fpn_bottleneck", 0, 2048)]


def conv_case(i, cin):
    h, w = GRIDS[i]
    M = B * h * w
    x = torch.randn(B, h, w, cin, device=dev).to(bf)
    Wt = (torch.randn(1, Ch, 9 * cin, device=dev) * 0.02).to(bf)
    Wg = torch.zeros(1, Ch, 9 * cin, device=dev)
    dy = torch.randn(1, M, Ch, device=dev).to(bf)
    return x, Wt, Wg, dy, (1, B, h, w, cin, 3, 3, 1, 1, h, w, False), M


if "convs" in PARTS:
    print("the five 3x3 convs, bf16 (forward; input gradient = flip + implicit conv; weight gradient = grouped launch):")
    for name, i, cin in CONVS:
        x, Wt, Wg, dy, geom, M = conv_case(i, cin)
        gmac = M * 9 * cin * Ch / 1e9
        with torch.no_grad():
            report(f"{name} fwd  ", lambda _: F.ConvF.apply(x, Wt, Wg, None, None, geom, None), gmac=gmac, n=20, warm=3)
        report(f"{name} dgrad", lambda _: F._conv_dgrad_implicit(dy, Wt, geom), gmac=gmac, n=20, warm=3)

        def wgrad(_):
            assert deferred.conv_wgrad(dy, x, Wg, None, geom[:11])
            deferred.flush()

        report(f"{name} wgrad", wgrad, gmac=gmac, n=20, warm=3)
        del x, Wt, Wg, dy
        torch.cuda.empty_cache()

if "dgrad" in PARTS:
    name, i, cin = CONVS[1]
    x, Wt, Wg, dy, geom, M = conv_case(i, cin)
    print(f"{name}'s input gradient both ways ({M} rows, 512 -> 512):")

    def old(_):
        dcols = F._dgrad(dy, Wt, torch.empty(1, M, 9 * cin, dtype=bf, device=dev))
        dx = torch.empty(B, *GRIDS[i], cin, dtype=bf, device=dev)
        K.call("cmx_col2im_nhwc", dcols, dx, B, *GRIDS[i], cin, 3, 3, 1, 1, *GRIDS[i], 9 * cin, 1)

    report(f"flip + implicit conv (allocates the flipped weights, {2 * Wt.numel() / 1e6:.1f} MB)",
           lambda _: F._conv_dgrad_implicit(dy, Wt, geom), n=20, warm=3)
    report(f"dcols GEMM + col2im (allocates dcols, {2 * M * 9 * cin / 1e6:.0f} MB)", old, n=20, warm=3)

if "head" in PARTS:
    head, store = make_head()
    head.train()
    feats = [rows(i, c).requires_grad_(True) for i, c in enumerate(CH)]
    dout = torch.randn(B * 120 * 160, KC, device=dev).to(bf)

    def run(i):
        head.run(store, feats, GRIDS, B, True).backward(dout)
        deferred.flush()

    def fwd(i):
        with torch.no_grad():
            head.run(store, feats, GRIDS, B, True)

    print(f"head forward + backward, eager: {launches(run)} library launches")
    report("forward + backward", run, n=10, warm=2)
    report("forward alone", fwd, n=10, warm=2)
    del head, store, feats
    torch.cuda.empty_cache()

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

    new, old = "UPerHead + aux head", "MLPDecoder"
    steps = {old: make_step(), new: make_step(decoder="UPerHead")}
    for rep in range(ROUNDS):
        for order in ((old, new), (new, old)):
            t = {name: timed(lambda i: steps[name][0].replay(), 10, warm=3) / 1e3 for name in order}
            print(f"round {rep} captured step, {order[0]} first: " + ", ".join(f"{n} {t[n]:.3f} ms" for n in sorted(t)),
                  flush=True)
    for name, (_, loss, nl, _) in steps.items():
        print(f"{name}: {nl} library launches per eager step (C-ABI calls seen by _lib.observer); loss after the "
              f"replays {loss.item():.4f}; peak memory {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")
