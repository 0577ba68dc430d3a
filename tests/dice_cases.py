"""Case table and fp64 references of DiceLoss / DiceCELoss on the fused upsample + loss path
(cmx_upsample_dice_fwd_adj; functions.UpsampleDiceF), shared by tests/test_dice_cases.py (CPU) and
tests/test_gpu_dice.py.  Shapes, inputs, the autograd reference and the bounds are those of
tests/loss_cases.py; the reference is the plain-PyTorch restatement in utils/loss_opr.py in fp64.
"""
from __future__ import annotations

import functools
import os
import sys

import torch
import torch.nn.functional as Fn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from loss_cases import SHAPES, BIG, make_inputs, reference_of, relerr, TOL, LOSS_TOL, IGNORE, DLOSS  # noqa: E402,F401

SMOOTH = 1e-6
# name -> alpha of DiceCELoss; 1.0 = pure DiceLoss.  Pure Dice is in every sweep: at the training
# shape its gradient is a few percent of CE's, so a missing Dice term would hide inside the 16-bit
# bound of a DiceCE case.
CRITERIA = {"dice": 1.0, "dice_ce": 0.5, "dice_ce_a0.9": 0.9}
PER_IMAGE_SHAPE = SHAPES[2]


def make_criterion(name):
    """The criterion object as a user hands it to EncoderDecoder."""
    from rgbx_semantic_segmentation_amd.utils.loss_opr import DiceCELoss, DiceLoss
    alpha = CRITERIA[name]
    if alpha == 1.0:
        return DiceLoss(smooth=SMOOTH, ignore_index=IGNORE, reduction="mean")
    return DiceCELoss(alpha=alpha, ignore_index=IGNORE, reduction="mean")


@functools.lru_cache(maxsize=None)
def expected(name, shape, dtype, kind="gauss", ignored="rect"):
    """The reference on the logits as the kernel sees them: rounded to the storage dtype."""
    lg, lab = make_inputs(shape, kind, ignored)
    return reference_of(make_criterion(name), lg.to(dtype).double(), lab)


def per_image_inputs():
    """PER_IMAGE_SHAPE: image 0 labelled with classes {0, 1} only (17 classes have T = 0 and a dice
    of smooth / (P + smooth)), image 1 ignored except one pixel (U of a class there is one pixel's
    p_k): statistics shared between the images, or a wrong image's coefficients, move the result."""
    lg, lab = make_inputs(PER_IMAGE_SHAPE, ignored="none")
    lab[0] = lab[0] % 2
    lab[1] = IGNORE
    lab[1, 21, 30] = 5
    return lg, lab


@functools.lru_cache(maxsize=None)
def expected_per_image(name):
    lg, lab = per_image_inputs()
    return reference_of(make_criterion(name), lg, lab)


def upsampled(lg):
    """(B, K, 4h, 4w) fp64: the x4 bilinear upsample of low-res logits (B, h, w, K)."""
    return Fn.interpolate(lg.double().permute(0, 3, 1, 2), scale_factor=4, mode="bilinear", align_corners=False)


def stats_reference(lg, lab):
    """(B, K, 3) fp64 = I, P, T of the fp64 softmax of the upsampled logits, and the valid count (B)."""
    K = lg.shape[3]
    p = torch.softmax(upsampled(lg), dim=1)
    valid = (lab != IGNORE).unsqueeze(1).double()
    onehot = Fn.one_hot(lab.clamp(0, K - 1), K).movedim(-1, 1).double() * valid
    p = p * valid
    return torch.stack([(p * onehot).sum((2, 3)), p.sum((2, 3)), onehot.sum((2, 3))], -1), valid.sum((1, 2, 3))


def uniform_dice_loss(lab, K, smooth=SMOOTH):
    """All-zero logits: p_k = 1/K at every pixel, so with n_b valid pixels and T the label
    histogram, dice[b, k] = (2 T / K + s) / (n_b / K + T + s), from the labels alone."""
    valid = lab != IGNORE
    T = torch.stack([torch.bincount(lab[b][valid[b]].clamp(0, K - 1), minlength=K) for b in range(lab.shape[0])])
    T = T.double()
    n = valid.flatten(1).sum(1, keepdim=True).double()
    return (1 - ((2 * T / K + smooth) / (n / K + T + smooth)).mean()).item()
