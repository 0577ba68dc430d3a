"""Case table and fp64 reference of the fused upsample + loss family (cmx_upsample_loss_fwd_adj;
functions.UpsampleLossF), shared by tests/test_loss_cases.py (CPU) and tests/test_gpu_loss.py.

The reference is the plain-PyTorch restatement in rgbx_semantic_segmentation_amd/utils/loss_opr.py
(and torch's own CrossEntropyLoss) evaluated in fp64 on F.interpolate(x4, bilinear,
align_corners=False) of the low-resolution logits, differentiated by torch autograd.  It is
computed once per (criterion, shape, input kind, storage dtype) and shared; nothing mutates it.
"""
from __future__ import annotations

import functools
import math
from collections import namedtuple

import torch
import torch.nn as nn
import torch.nn.functional as Fn

IGNORE = 255
DLOSS = 0.7
ALPHA = 0.25

# name -> (kind, gamma): kind in focal | ce_focal | wce | fl2d | fl2d_w
CRITERIA = {
    "focal_g0": ("focal", 0.0), "focal_g1": ("focal", 1.0), "focal_g2": ("focal", 2.0), "focal_g4": ("focal", 4.0),
    "focal_g2.5": ("focal", 2.5), "ce_focal": ("ce_focal", 4.0), "wce": ("wce", 0.0), "fl2d": ("fl2d", 0.0),
    "fl2d_w": ("fl2d_w", 0.0),
}
# (B, h, w, K): the smallest shapes that reach every edge of the kernel's 6 x 8 low-res tiling
SHAPES = [(1, 5, 7, 40),        # one partial tile, the full class count
          (1, 15, 20, 9),       # ragged in both directions, 31 padded classes
          (2, 13, 17, 19)]      # batch stride, ragged
BIG = (2, 120, 160, 40)         # the B2 training shape (FocalLoss gamma 4, bf16 only)

# the bounds of tests/test_gpu_kernels.py::test_upsample_ce
TOL = {torch.float32: 1e-4, torch.bfloat16: 3e-2, torch.float16: 3e-2}
LOSS_TOL = {torch.float32: 1e-5, torch.bfloat16: 1e-2, torch.float16: 1e-2}


def class_weights(K):
    return 0.5 + 0.37 * (torch.arange(K) % 5).float()


def make_criterion(name, K):
    """The criterion object(s) as a user hands them to EncoderDecoder."""
    from rgbx_semantic_segmentation_amd.utils.loss_opr import FocalLoss, FocalLoss2d
    kind, gamma = CRITERIA[name]
    if kind == "focal":
        return FocalLoss(ignore_label=IGNORE, gamma=gamma, alpha=ALPHA, reduction="mean")
    if kind == "ce_focal":
        return (nn.CrossEntropyLoss(reduction="mean", ignore_index=IGNORE),
                FocalLoss(ignore_label=IGNORE, gamma=gamma, alpha=ALPHA, reduction="mean"))
    if kind == "wce":
        return nn.CrossEntropyLoss(weight=class_weights(K), reduction="mean", ignore_index=IGNORE)
    if kind == "fl2d":
        return FocalLoss2d(ignore_index=IGNORE, reduction="mean")
    return FocalLoss2d(weight=class_weights(K).tolist(), ignore_index=IGNORE, reduction="mean")


class Restated(nn.Module):
    """A criterion (or the CE_Focal pair) as one callable on full-resolution logits, in the
    logits' dtype: CE_Focal = CE + 0.2 * Focal (reference builder.py:246-247)."""

    def __init__(self, criterion):
        super().__init__()
        self.pair = isinstance(criterion, (tuple, list))
        self.parts = nn.ModuleList(list(criterion) if self.pair else [criterion])

    def forward(self, pred, target):
        for m in self.parts.modules():                # class weights follow the logits' dtype
            for k, b in list(m._buffers.items()):
                if b is not None and b.dtype != pred.dtype:
                    m._buffers[k] = b.to(pred.dtype)
        if self.pair:
            return self.parts[0](pred, target) + 0.2 * self.parts[1](pred, target)
        return self.parts[0](pred, target)


def make_inputs(shape, kind="gauss", ignored="rect", seed=7):
    """Low-res logits (B, h, w, K) fp64 and labels (B, 4h, 4w), as test_upsample_ce draws them:
    randn * 3 and an ignored rectangle.  kind uniform: all-zero logits; ignored all / none / rect."""
    B, h, w, K = shape
    g = torch.Generator().manual_seed(seed)
    lg = torch.randn(B, h, w, K, dtype=torch.float64, generator=g) * 3
    if kind == "uniform":
        lg.zero_()
    lab = torch.randint(0, K, (B, 4 * h, 4 * w), generator=g)
    if ignored == "rect":
        lab[:, 5:30, 7:40] = IGNORE
    elif ignored == "all":
        lab.fill_(IGNORE)
    return lg, lab


Ref = namedtuple("Ref", "loss dlogits gsum")


def reference_of(criterion, lg, lab, dloss=DLOSS):
    """fp64: loss, d(dloss * loss)/d(low-res logits) (B, h, w, K), and gsum (K) = the same gradient
    w.r.t. the full-resolution logits summed over all pixels (the bilinear adjoint conserves it)."""
    x = lg.double().clone().requires_grad_(True)
    up = Fn.interpolate(x.permute(0, 3, 1, 2), scale_factor=4, mode="bilinear", align_corners=False)
    up.retain_grad()
    loss = Restated(criterion)(up, lab)
    (loss * dloss).backward()
    return Ref(loss.detach(), x.grad.detach(), up.grad.detach().sum(dim=(0, 2, 3)))


@functools.lru_cache(maxsize=None)
def expected(name, shape, dtype, kind="gauss", ignored="rect"):
    """The reference on the logits as the kernel sees them: rounded to the storage dtype."""
    lg, lab = make_inputs(shape, kind, ignored)
    return reference_of(make_criterion(name, shape[3]), lg.to(dtype).double(), lab)


def uniform_focal_loss(K, gamma, alpha=ALPHA, eps=1e-8):
    """Per valid pixel at p_k = 1/K for every k (all-zero logits)."""
    p = 1.0 / K
    return alpha * (1 - p) ** gamma * -math.log(p + eps) + (K - 1) * (1 - alpha) * p ** gamma * -math.log(1 - p + eps)


def relerr(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()
