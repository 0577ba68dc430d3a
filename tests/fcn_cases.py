"""Case table and fp64 reference of the fused upsample + loss at the scales of an FCN head
(cmx_upsample_loss_scaled_fwd_adj; functions.UpsampleScaledLossF), shared by tests/test_fcn_cases.py (CPU)
and tests/test_gpu_fcn_loss.py.

The reference is loss_cases' restatement (utils/loss_opr.py and torch's own CrossEntropyLoss) evaluated in
fp64 on F.interpolate(scale_factor=S, bilinear, align_corners=False) of the low-resolution logits,
differentiated by torch autograd.  The bounds are loss_cases' (imported, not copied): relative loss error
< LOSS_TOL[dtype], relerr(dlogits) < 2 TOL[dtype]; the reference of a 16-bit run takes the rounded logits.
It is computed once per (criterion, S, shape, input kind, storage dtype) and shared; nothing mutates it.
"""
from __future__ import annotations

import functools
import os
import sys

import torch
import torch.nn as nn
import torch.nn.functional as Fn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from loss_cases import (ALPHA, CRITERIA, DLOSS, IGNORE, LOSS_TOL, TOL, Ref, Restated, make_criterion,  # noqa: E402,F401
                        relerr, uniform_focal_loss)

SCALES = (8, 16, 32)
PLAIN_CE = "ce"
NAMES = [PLAIN_CE] + list(CRITERIA)
# (B, h, w, K)
SHAPES = [(1, 1, 1, 5),         # every tap clamps: the upsample is a broadcast
          (1, 1, 4, 9),         # rows are a pure broadcast
          (1, 3, 1, 9),         # columns are a pure broadcast
          (2, 4, 5, 40),        # the batch stride and the full class count
          (1, 7, 9, 9)]         # ragged against the cells of a workgroup (16 / 4 / 1 per row), 31 padded classes
# the shapes of the CPU check of the bounds (test_fcn_cases.py)
CPU_SHAPES = [(1, 1, 1, 5), (2, 4, 5, 40), (1, 7, 9, 9), (2, 15, 20, 19)]


def criterion_of(name, K):
    """The criterion object(s) as a user hands them to EncoderDecoder; "ce" is the default plain CE."""
    if name == PLAIN_CE:
        return nn.CrossEntropyLoss(reduction="mean", ignore_index=IGNORE)
    return make_criterion(name, K)


def make_inputs(shape, S, kind="gauss", ignored="rect", seed=7):
    """Low-res logits (B, h, w, K) fp64 and labels (B, S h, S w), drawn as loss_cases.make_inputs draws them
    (randn * 3, an ignored rectangle); the rectangle [5:30, 7:40) of the x4 cases scales with S / 4, so it
    covers the same share of the image and crosses cell borders in both directions."""
    B, h, w, K = shape
    g = torch.Generator().manual_seed(seed)
    lg = torch.randn(B, h, w, K, dtype=torch.float64, generator=g) * 3
    if kind == "uniform":
        lg.zero_()
    lab = torch.randint(0, K, (B, S * h, S * w), generator=g)
    if ignored == "rect":
        f = S // 4
        lab[:, 5 * f:30 * f, 7 * f:40 * f] = IGNORE      # starts at row 1.25 S: a one-row map has none ignored
    elif ignored == "all":
        lab.fill_(IGNORE)
    return lg, lab


def reference_of(criterion, lg, lab, S, dloss=DLOSS, dtype=torch.float64):
    """loss, d(dloss * loss)/d(low-res logits) (B, h, w, K), and gsum (K) = the same gradient w.r.t. the
    full-resolution logits summed over all pixels (the bilinear adjoint conserves it); fp64 by default."""
    x = lg.to(dtype).clone().requires_grad_(True)
    up = Fn.interpolate(x.permute(0, 3, 1, 2), scale_factor=S, mode="bilinear", align_corners=False)
    up.retain_grad()
    loss = Restated(criterion)(up, lab)
    (loss * dloss).backward()
    return Ref(loss.detach(), x.grad.detach(), up.grad.detach().sum(dim=(0, 2, 3)))


@functools.lru_cache(maxsize=None)
def expected(name, S, shape, dtype, kind="gauss", ignored="rect"):
    """The reference on the logits as the kernel sees them: rounded to the storage dtype."""
    lg, lab = make_inputs(shape, S, kind, ignored)
    return reference_of(criterion_of(name, shape[3]), lg.to(dtype).double(), lab, S)
