"""Time the MLPDecoderpp channel-attention gate at the B2 480 x 640 bs=2 shape, (B, N, C) =
(2, 19200, 512) bf16:

* each of the four se_gate.hip kernels standalone, HIP events around 200 launches after 10
  warm-up launches, twice: on ONE set of buffers (78 MB of traffic fits the 256 MB Infinity
  Cache, so this is the in-step, cache-warm figure) and rotating over 8 buffer sets (630 MB, the
  HBM figure).  Prints us per launch, TB/s of the algorithmic bytes and the share of 8 TB/s;
* the gate forward + backward, functions.SEGateF beside the same gate in eager PyTorch;
* the decode head forward + backward (B2 channels, E = 512, K = 40), MLPDecoder and
  MLPDecoderpp alternating in one process.
Usage: python scripts/bench_decoder.py [rounds]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rgbx_semantic_segmentation_amd import deferred  # noqa: E402
from rgbx_semantic_segmentation_amd import functions as F  # noqa: E402
from rgbx_semantic_segmentation_amd._lib import call, ptr, query, stream  # noqa: E402
from rgbx_semantic_segmentation_amd.models.decoders import MLPDecoder, MLPDecoderpp  # noqa: E402
from rgbx_semantic_segmentation_amd.params import ParamStore  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
PEAK_TBS = 8.0
B, N, C, DT = 2, 19200, 512, 1
NSETS = 8
dev = torch.device("cuda", 0)
NSL = query("cmx_small_linear_nslice")


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


# ------------------------------------------------------------------ the four kernels
ys = [torch.randn(B, N, C, device=dev).to(torch.bfloat16) for _ in range(NSETS)]
ds_ = [torch.randn(B, N, C, device=dev).to(torch.bfloat16) for _ in range(NSETS)]
outs = [torch.empty(B, N, C, dtype=torch.bfloat16, device=dev) for _ in range(NSETS)]
a = torch.rand(B, C, device=dev)
dsc = (torch.rand(B, C, device=dev) > 0.1).float() / 0.9
pooled = torch.empty(B, C, device=dev)
ws = torch.empty(query("cmx_se_pool_workspace", B, N, C) // 4, device=dev)
tk = torch.zeros(query("cmx_se_pool_tickets", B, C), dtype=torch.int32, device=dev)
dap = torch.empty(query("cmx_se_bwd_nslice", B, N, C), B, C, device=dev)
dpp = torch.randn(NSL, B, C, device=dev)
act = B * N * C * 2
KERNELS = (
    ("se_pool_fwd", act, lambda i: call("cmx_se_pool_fwd", ptr(ys[i]), ptr(pooled), ptr(ws), ptr(tk), B, N, C, DT,
                                        stream())),
    ("se_scale_fwd", 2 * act, lambda i: call("cmx_se_scale_fwd", ptr(ys[i]), ptr(a), ptr(dsc), ptr(outs[i]), B, N, C,
                                             DT, stream())),
    ("se_bwd_reduce", 2 * act, lambda i: call("cmx_se_bwd_reduce", ptr(ds_[i]), ptr(ys[i]), ptr(dsc), ptr(dap), B, N,
                                              C, DT, stream())),
    ("se_bwd_apply", 2 * act, lambda i: call("cmx_se_bwd_apply", ptr(ds_[i]), ptr(a), ptr(dsc), ptr(dpp), NSL, B * C,
                                             ptr(outs[i]), B, N, C, DT, stream())),
)
for rep in range(ROUNDS):
    for name, nbytes, run in KERNELS:
        for label, pick in (("one set (cache-warm)", lambda i: 0), (f"{NSETS} sets (HBM)", lambda i: i % NSETS)):
            us = timed(lambda i: run(pick(i)), 200)
            tbs = nbytes / us / 1e6
            print(f"round {rep} {name:14s} {label:22s} {nbytes / 1e6:5.1f} MB: {us:7.1f} us  {tbs:5.2f} TB/s  "
                  f"{tbs / PEAK_TBS:4.2f} of {PEAK_TBS:g} TB/s")
assert not bool(tk.any())

# ------------------------------------------------------------------ the gate: SEGateF beside eager PyTorch
H = C // 4
W1 = torch.nn.Parameter(torch.randn(H, C, device=dev) / C ** 0.5)
b1 = torch.nn.Parameter(torch.zeros(H, device=dev))
W2 = torch.nn.Parameter(torch.randn(C, H, device=dev) / H ** 0.5)
b2 = torch.nn.Parameter(torch.zeros(C, device=dev))
prm = {"w": (W1.data, b1.data, W2.data, b2.data), "g": tuple(torch.zeros_like(p) for p in (W1, b1, W2, b2))}
yq = ys[0].clone().requires_grad_(True)
dout = ds_[0]


def gate_hip(i):
    F.SEGateF.apply(yq, prm, dsc, W1).backward(dout)


def gate_eager(i):
    pooled = yq.float().mean(1)
    g = torch.sigmoid(torch.nn.functional.gelu(pooled @ W1.t() + b1) @ W2.t() + b2)
    (yq * (g * dsc).to(yq.dtype)[:, None, :]).backward(dout)


for rep in range(ROUNDS):
    for name, run in (("SEGateF fwd+bwd", gate_hip), ("eager torch fwd+bwd", gate_eager)):
        print(f"round {rep} gate {name:20s}: {timed(run, 50, warm=5):8.1f} us")


# ------------------------------------------------------------------ the heads, alternating
CH, E, K = (64, 128, 320, 512), 512, 40
GRIDS = [(120, 160), (60, 80), (30, 40), (15, 20)]


def make_head(cls):
    torch.manual_seed(0)
    head = cls(CH, K, embed_dim=E)
    for mod in head.modules():
        for k, b in list(mod._buffers.items()):
            if b is not None:
                mod._buffers[k] = b.to(dev)
    return head, ParamStore(head, dev, torch.bfloat16)


heads = {"MLPDecoder": make_head(MLPDecoder.DecoderHead), "MLPDecoderpp": make_head(MLPDecoderpp.DecoderHead)}
feats = [torch.randn(B, h * w, c, device=dev).to(torch.bfloat16).requires_grad_(True) for c, (h, w) in zip(CH, GRIDS)]
d2 = (torch.rand(B, E, device=dev) > 0.1).float() / 0.9
dlog = torch.randn(B * GRIDS[0][0] * GRIDS[0][1], K, device=dev).to(torch.bfloat16)


def head_step(name):
    head, store = heads[name]

    def run(i):
        head.run(store, feats, GRIDS, B, True, dscale=d2).backward(dlog)
        deferred.flush()
    return run


for rep in range(ROUNDS):
    for name in heads:
        print(f"round {rep} head {name:13s} fwd+bwd: {timed(head_step(name), 20, warm=3):8.1f} us")
