"""Standalone DWConv timing at the B2 480x640 bs=2 shapes (G=2 streams): fwd_save and
bwd_saved, HIP-event timed over graph-captured repeats, with algorithmic GB/s.
Usage (GPU box): python scripts/bench_dw.py"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rgbx_semantic_segmentation_amd import kernels as Kn  # noqa: E402


def timeit(fn, iters=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        for _ in range(iters):
            fn()
    g.replay()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    g.replay()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3


def main():
    G, B = 2, 2
    for (H, W, C) in [(120, 160, 256), (60, 80, 512), (30, 40, 1280), (15, 20, 2048)]:
        NI = G * B
        h = torch.randn(NI, H * W, C, device="cuda").bfloat16()
        w = torch.randn(G, C, 9, device="cuda") * 0.3
        b = torch.randn(G, C, device="cuda") * 0.1
        out, gp, da, dh = (torch.empty_like(h) for _ in range(4))
        da.normal_()
        ws = Kn._ws(Kn.query("cmx_dwconv3x3_bwd_workspace", NI, B, H, W, C), h.device)
        dw = torch.empty(G, C, 9, device="cuda")
        db = torch.empty(G, C, device="cuda")
        ACT = Kn.ACT["gelu"]

        def fwd():
            Kn.call("cmx_dwconv3x3_fwd_save", Kn.ptr(h), Kn.ptr(w), Kn.ptr(b), Kn.ptr(out), Kn.ptr(gp), NI, B, H, W,
                    C, ACT, 1, Kn.stream())

        def bwd():
            Kn.call("cmx_dwconv3x3_bwd_saved", Kn.ptr(da), Kn.ptr(h), Kn.ptr(gp), Kn.ptr(w), Kn.ptr(dh), Kn.ptr(dw),
                    Kn.ptr(db), Kn.ptr(ws), NI, B, H, W, C, 0, 1, Kn.stream())
        tf, tb = timeit(fwd), timeit(bwd)
        nb = h.numel() * 2
        print(f"H{H} W{W} C{C}: fwd_save {tf:7.1f} us {3 * nb / tf / 1e3:6.0f} GB/s   "
              f"bwd_saved(+reduce) {tb:7.1f} us {4 * nb / tb / 1e3:6.0f} GB/s  (tensor {nb / 1e6:.1f} MB)")
        if C // 4 in (64, 128):
            mlp_fused(G, B, H, W, C // 4, C, h, w, b, out, gp, dh, dw, db, ws, tf, tb)


def mlp_fused(G, B, H, W, C, hidden, f0, w, b, out, gp, dh, dw, db, ws, tf, tb):
    """Stages 1-2: fc1 + the forward and fc2's dgrad + the backward as the two launches of today (GEMM, then the
    depthwise kernel timed above) against the one launch of cmx_mlp_fc1_dwconv_fwd / cmx_mlp_fc2_dwconv_bwd."""
    NI, M = G * B, B * H * W
    x = torch.randn(G, M, C, device="cuda").bfloat16()
    dz = torch.randn(G, M, C, device="cuda").bfloat16()
    W1 = (torch.randn(G, hidden, C, device="cuda") * C ** -0.5).bfloat16()
    W2 = (torch.randn(G, C, hidden, device="cuda") * hidden ** -0.5).bfloat16()
    b1 = torch.randn(G, hidden, device="cuda") * 0.1
    f0v, da = f0.view(G, M, hidden), torch.empty(G, M, hidden, device="cuda", dtype=torch.bfloat16)
    ACT = Kn.ACT["gelu"]
    t_fc1 = timeit(lambda: Kn.gemm(x, W1, f0v, bias=b1))
    t_dg = timeit(lambda: Kn.gemm(dz, W2.transpose(1, 2), da))
    t_ff = timeit(lambda: Kn.call("cmx_mlp_fc1_dwconv_fwd", x, W1, b1, w, b, f0, out, gp, NI, B, H, W, C, hidden, ACT, 1))
    t_fb = timeit(lambda: Kn.call("cmx_mlp_fc2_dwconv_bwd", dz, W2, f0, gp, w, dh, dw, db, ws, NI, B, H, W, C, hidden,
                                  0, 1))
    nb = f0.numel() * 2
    print(f"   fc1 GEMM {t_fc1:6.1f} us + fwd_save = {t_fc1 + tf:6.1f} us | fused forward {t_ff:6.1f} us "
          f"{3 * nb / t_ff / 1e3:6.0f} GB/s")
    print(f"   fc2 dgrad GEMM {t_dg:6.1f} us + bwd_saved(+reduce) = {t_dg + tb:6.1f} us | fused backward(+reduce) "
          f"{t_fb:6.1f} us {3 * nb / t_fb / 1e3:6.0f} GB/s")


if __name__ == "__main__":
    main()
