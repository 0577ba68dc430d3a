"""Time the fused optimizer launches beside each other on a B2-sized flat buffer (66.58 M fp32
parameters + bf16 shadow): cmx_adamw_step, cmx_sgdm_step with momentum 0.9 and with momentum 0,
alternated in one process for several rounds, 3 warm-up launches and HIP events around 20
launches each.  Prints us per launch and TB/s of the algorithmic traffic (30, 22 and 14 B per
parameter) with its share of the 8 TB/s HBM peak."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rgbx_semantic_segmentation_amd._lib import call, ptr, stream  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
PEAK_TBS = 8.0

n = 66_580_480
p = torch.randn(n, device="cuda") * 0.02
g = torch.randn(n, device="cuda") * 1e-3
m = torch.zeros(n, device="cuda")
v = torch.zeros(n, device="cuda")
sh = torch.empty(n, dtype=torch.bfloat16, device="cuda")
dec = torch.ones(n // 64, dtype=torch.uint8, device="cuda")
lr = torch.full((1,), 6e-5, device="cuda")
step = torch.zeros(1, device="cuda")


def adamw():
    call("cmx_adamw_step", ptr(p), ptr(g), ptr(m), ptr(v), ptr(sh), 1, ptr(dec), n, ptr(lr), ptr(step), 0.9, 0.999,
         1e-8, 0.01, 1.0, 0, stream())


def sgdm():
    call("cmx_sgdm_step", ptr(p), ptr(g), ptr(m), ptr(sh), 1, ptr(dec), n, ptr(lr), 0.9, 0.01, 0, 1.0, 0, 0, 0,
         stream())


def sgd0():
    call("cmx_sgdm_step", ptr(p), ptr(g), 0, ptr(sh), 1, ptr(dec), n, ptr(lr), 0.0, 0.01, 0, 1.0, 0, 0, 0, stream())


for rep in range(ROUNDS):
    for name, run, nbytes in (("adamw_step", adamw, 30.0), ("sgdm_step mu=0.9", sgdm, 22.0),
                              ("sgdm_step mu=0", sgd0, 14.0)):
        for _ in range(3):
            run()
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(20):
            run()
        e.record()
        torch.cuda.synchronize()
        us = s.elapsed_time(e) / 20 * 1e3
        tbs = nbytes * n / us / 1e6
        print(f"round {rep} {name:17s} {nbytes:2.0f} B/param: {us:7.1f} us  {tbs:5.2f} TB/s  "
              f"{tbs / PEAK_TBS:4.2f} of {PEAK_TBS:g} TB/s")
