"""The criteria beside ``nn.CrossEntropyLoss`` that the fused upsample + loss kernels cover
(reference: utils/loss_opr.py; selected by train.py:70-88), with the reference's constructor
signatures at the reference's import path.

On the training hot path ``EncoderDecoder`` never calls these modules' ``forward``: it reads
their hyper-parameters and runs ``cmx_upsample_loss_fwd_adj`` on the low-resolution logits
(functions.UpsampleLossF; DiceLoss / DiceCELoss: ``cmx_upsample_dice_fwd_adj``,
functions.UpsampleDiceF; ProbOhemCrossEntropy2d: ``cmx_upsample_ohem_fwd_adj``,
functions.UpsampleOhemF).  ``forward(pred, target)`` is the plain-PyTorch statement of the same
math on full-resolution logits (B, K, H, W): API compatibility off the hot path, and the tests'
fp64 reference.  ``focal_grad`` / ``focal2d_grad`` / ``dice_grad`` are the closed-form gradients
the kernels implement.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

FOCAL_EPS = 1e-8
CE_FOCAL_WEIGHT = 0.2       # CE_Focal: loss = CE + 0.2 * Focal (reference builder.py:246-247)


def check_focal_gamma(gamma) -> float:
    """The kernels take gamma == 0 or gamma >= 1 (x^(gamma-1) of the gradient is unbounded at
    x = 0 in between)."""
    g = float(gamma)
    if not (g == 0.0 or g >= 1.0):
        raise ValueError(f"FocalLoss gamma={gamma!r}: only gamma == 0 or gamma >= 1 is supported")
    return g


class FocalLoss(nn.Module):
    """Sum over ALL K classes per pixel of -a_k (1 - pt_k)^gamma log(pt_k + 1e-8), with
    pt_k = p_k, a_k = alpha at the target class and pt_k = 1 - p_k, a_k = 1 - alpha elsewhere;
    mean = sum over valid pixels / (n_valid + 1e-8), so nothing valid gives 0, not NaN.
    valid = (target != ignore_label); the class is clamp(target, 0, K - 1): an out-of-range
    label that is not the ignore value is clamped, not ignored."""

    def __init__(self, ignore_label, gamma=2.0, alpha=0.25, reduction='mean'):
        super().__init__()
        self.ignore_label = ignore_label
        self.gamma = gamma
        self.alpha = alpha
        self.reduction = reduction

    def pixel_loss(self, pred, target):
        """(loss (B, H, W) summed over classes and zeroed at invalid pixels, valid mask)."""
        K = pred.shape[1]
        valid = target != self.ignore_label
        onehot = F.one_hot(target.clamp(0, K - 1), K).movedim(-1, 1).bool()
        p = torch.softmax(pred, dim=1)
        pt = torch.where(onehot, p, 1 - p)
        a = torch.where(onehot, torch.full_like(p, self.alpha), torch.full_like(p, 1 - self.alpha))
        loss = -a * (1 - pt) ** self.gamma * torch.log(pt + FOCAL_EPS)
        return loss.sum(1) * valid.to(loss.dtype), valid

    def forward(self, pred, target):
        loss, valid = self.pixel_loss(pred, target)
        if self.reduction == 'mean':
            return loss.sum() / (valid.to(loss.dtype).sum() + FOCAL_EPS)
        if self.reduction == 'sum':
            return loss.sum()
        return loss.flatten(1)


class FocalLoss2d(nn.Module):
    """NLLLoss of (1 - p)^2 log p.  The exponent is the reference's hard-coded 2: the
    constructor's ``gamma`` is stored and otherwise IGNORED, as in the reference.  ``weight``: a
    sequence of K class weights (NLLLoss's weighted mean), or None."""

    def __init__(self, gamma=0, weight=None, reduction='mean', ignore_index=255):
        super().__init__()
        self.gamma = gamma
        w = None if weight is None else torch.as_tensor(weight, dtype=torch.float32).flatten().clone()
        self.loss = nn.NLLLoss(weight=w, reduction=reduction, ignore_index=ignore_index)

    def forward(self, input, target):
        return self.loss((1 - F.softmax(input, 1)) ** 2 * F.log_softmax(input, 1), target)


def _dice_terms(pred, target, ignore_index):
    """(p masked, onehot masked) (B, K, H, W) in pred's dtype: the softmax and the one-hot of
    clamp(target, 0, K - 1), both zeroed where target == ignore_index (FocalLoss's label rule)."""
    K = pred.shape[1]
    valid = (target != ignore_index).unsqueeze(1).to(pred.dtype)
    onehot = F.one_hot(target.clamp(0, K - 1), K).movedim(-1, 1).to(pred.dtype)
    return torch.softmax(pred, dim=1) * valid, onehot * valid


class DiceLoss(nn.Module):
    """1 - dice, dice[b, k] = (2 I + smooth) / (P + T + smooth) with, per image b and class k over
    the valid pixels, I = sum p_k [y = k], P = sum p_k, T = sum [y = k]; 'mean' / 'sum' reduce
    dice over (b, k), anything else returns 1 - dice (B, K).  Nothing valid: every dice is 1."""

    def __init__(self, smooth=1e-6, ignore_index=255, reduction='mean'):
        super().__init__()
        self.smooth = smooth
        self.ignore_index = ignore_index
        self.reduction = reduction

    def forward(self, preds, targets):
        p, onehot = _dice_terms(preds, targets, self.ignore_index)
        inter = (p * onehot).sum(dim=(2, 3))
        union = p.sum(dim=(2, 3)) + onehot.sum(dim=(2, 3))
        dice = (2 * inter + self.smooth) / (union + self.smooth)
        if self.reduction == 'mean':
            return 1 - dice.mean()
        if self.reduction == 'sum':
            return 1 - dice.sum()
        return 1 - dice


class DiceCELoss(nn.Module):
    """alpha * DiceLoss + (1 - alpha) * nn.CrossEntropyLoss, both with the same ignore_index and
    reduction."""

    def __init__(self, alpha=0.5, ignore_index=255, reduction='mean'):
        super().__init__()
        self.alpha = alpha
        self.dice = DiceLoss(ignore_index=ignore_index, reduction=reduction)
        self.ce = nn.CrossEntropyLoss(ignore_index=ignore_index, reduction=reduction)

    def forward(self, preds, targets):
        return self.alpha * self.dice(preds, targets) + (1 - self.alpha) * self.ce(preds, targets)


class ProbOhemCrossEntropy2d(nn.Module):
    """Online hard example mining on plain CrossEntropyLoss: the mean of -log p_y over the KEPT pixels.
    valid = (target != ignore_label and 0 <= target < K) -- a label outside [0, K) counts as ignored, as
    the fused plain-CE path does; p_y = the softmax probability of the pixel's own class.
      min_kept > n_valid, min_kept <= 0 or n_valid == 0: nothing is filtered, the result is
        CrossEntropyLoss(mean) (NaN when nothing is valid);
      otherwise threshold = max(thresh, min_kept-th smallest p_y over the valid pixels) and
        kept = valid and p_y <= threshold: ties at the threshold are all kept.
    The mask is a constant for autograd.  ``down_ratio`` is stored and unused, as in the reference;
    ``use_weight=True`` (the reference's 19-entry Cityscapes table) is not carried over."""

    def __init__(self, ignore_label, reduction='mean', thresh=0.6, min_kept=256, down_ratio=1, use_weight=False):
        super().__init__()
        if use_weight:
            raise NotImplementedError("ProbOhemCrossEntropy2d(use_weight=True): the class-weight table is not supported")
        self.ignore_label = ignore_label
        self.thresh = float(thresh)
        self.min_kept = int(min_kept)
        self.down_ratio = down_ratio
        self.reduction = reduction
        self.criterion = nn.CrossEntropyLoss(reduction=reduction, ignore_index=ignore_label)

    @torch.no_grad()
    def selection(self, pred, target):
        """(kept mask (B, H, W), threshold, n_valid, n_below) of the rule above; threshold is +inf when
        nothing is filtered, n_below = #(valid and p_y <= thresh)."""
        K = pred.shape[1]
        valid = (target != self.ignore_label) & (target >= 0) & (target < K)
        py = torch.softmax(pred, dim=1).gather(1, target.clamp(0, K - 1).unsqueeze(1)).squeeze(1)
        pv = py[valid]
        n_valid = int(pv.numel())
        n_below = int((pv <= self.thresh).sum())
        if self.min_kept <= 0 or self.min_kept > n_valid:
            return valid, float("inf"), n_valid, n_below
        kth = pv.kthvalue(self.min_kept).values.item()
        threshold = kth if kth > self.thresh else self.thresh
        return valid & (py <= threshold), threshold, n_valid, n_below

    def forward(self, pred, target):
        kept = self.selection(pred, target)[0]
        return self.criterion(pred, torch.where(kept, target, torch.full_like(target, self.ignore_label)))


# ------------------------------------------------------------------ closed-form gradients
def dice_grad(z, target, ignore_index, smooth):
    """d(DiceLoss, mean)/dz for logits z (B, K, H, W): with U = P + T,
    u_k = v (c[b, k] - [y = k] a[b, k]), c = (2 I + s) / ((U + s)^2 B K), a = 2 / ((U + s) B K),
    dl/dz_j = p_j (u_j - sum_k u_k p_k); zero at ignored pixels."""
    B, K = z.shape[:2]
    valid = (target != ignore_index).unsqueeze(1).to(z.dtype)
    pm, onehot = _dice_terms(z, target, ignore_index)
    inter = (pm * onehot).sum(dim=(2, 3))
    union = pm.sum(dim=(2, 3)) + onehot.sum(dim=(2, 3))
    c = ((2 * inter + smooth) / ((union + smooth) ** 2 * B * K))[:, :, None, None]
    a = (2 / ((union + smooth) * B * K))[:, :, None, None]
    u = c * valid - a * onehot
    p = torch.softmax(z, dim=1)
    return p * (u - (u * p).sum(1, keepdim=True))



def focal_grad(z, target, ignore_label, gamma, alpha):
    """d(per-pixel FocalLoss)/dz for logits z (B, K, H, W), zero at invalid pixels (no 1/n):
    u_k = dl/dp_k, dl/dz_j = p_j (u_j - sum_k u_k p_k)."""
    K = z.shape[1]
    valid = (target != ignore_label).unsqueeze(1)
    onehot = F.one_hot(target.clamp(0, K - 1), K).movedim(-1, 1).bool()
    p = torch.softmax(z, dim=1)
    q = 1 - p
    x = torch.where(onehot, q, p)                     # 1 - pt
    y = torch.where(onehot, p, q) + FOCAL_EPS         # pt + eps
    a = torch.where(onehot, torch.full_like(p, alpha), torch.full_like(p, alpha - 1))
    u = -x ** gamma / y
    if gamma != 0:
        u = u + gamma * x ** (gamma - 1) * torch.log(y)
    u = a * u
    g = p * (u - (u * p).sum(1, keepdim=True))
    return g * valid.to(g.dtype)


def focal2d_grad(z, target, ignore_index, weight=None):
    """d(per-pixel w_y * -(1 - p_y)^2 log p_y)/dz = c (p - onehot),
    c = w_y ((1 - p_y)^2 - 2 p_y (1 - p_y) log p_y); zero at ignored pixels."""
    K = z.shape[1]
    valid = target != ignore_index
    t = torch.where(valid, target, torch.zeros_like(target))
    onehot = F.one_hot(t, K).movedim(-1, 1).to(z.dtype)
    lp = torch.log_softmax(z, dim=1)
    p = lp.exp()
    lpy = (lp * onehot).sum(1, keepdim=True)
    py = lpy.exp()
    c = (1 - py) ** 2 - 2 * py * (1 - py) * lpy
    if weight is not None:
        c = c * weight.to(z.dtype)[t].unsqueeze(1)
    return c * (p - onehot) * valid.unsqueeze(1).to(z.dtype)
