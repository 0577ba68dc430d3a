"""Case table and fp64 reference of ProbOhemCrossEntropy2d on the fused upsample + loss path
(cmx_upsample_ohem_fwd_adj / cmx_ohem_select; functions.UpsampleOhemF), shared by
tests/test_ohem_cases.py (CPU) and tests/test_gpu_ohem.py.

Inputs are loss_cases.make_inputs(shape) (gauss logits, an ignored rectangle, seed 7).  The reference
is the plain-PyTorch restatement (utils/loss_opr.ProbOhemCrossEntropy2d) in fp64 on the logits rounded
to the storage dtype and upsampled in fp64, through loss_cases.reference_of; it is computed once per
(case, dtype) and shared, and nothing mutates it.

MARGIN: the kernel's own p_y error is <= 2e-5 absolute (fp32 arithmetic on |z log2 e| < 32 has ulp
1.9e-6; two interpolation stages and the shift add a few ulps, exp2 and a 40-term sum about 1e-6
relative; p <= 1).  Every case keeps 5x that between the quantities that decide the kept set (see
margin_report), so the kept set is the same in fp32 and in fp64 and loss and gradient are comparable
at the family's bounds.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import torch
import torch.nn.functional as Fn

import loss_cases as lc

IGNORE, DLOSS = lc.IGNORE, lc.DLOSS
SHAPES, BIG = lc.SHAPES, lc.BIG
TOL, LOSS_TOL = lc.TOL, lc.LOSS_TOL
MARGIN = 1e-4
PY_TOL = 2e-5
SENTINEL = 2.0

Case = namedtuple("Case", "shape thresh min_kept n_valid n_below regime n_kept")
# regime: nofilter (nothing dropped), thresh (threshold = thresh), kth (threshold = the k-th smallest p_y)
CASES = {
    "s0_nofilter": Case(SHAPES[0], 0.6, 256, 245, 245, "nofilter", 245),
    "s0_minkept0": Case(SHAPES[0], 0.6, 0, 245, 245, "nofilter", 245),
    "s0_kth": Case(SHAPES[0], 0.021, 220, 245, 192, "kth", 220),
    "s1_thresh": Case(SHAPES[1], 0.6, 256, 3975, 3780, "thresh", 3780),
    "s1_thresh_low": Case(SHAPES[1], 0.07, 256, 3975, 2607, "thresh", 2607),
    "s1_kth": Case(SHAPES[1], 0.07, 3581, 3975, 2607, "kth", 3581),
    "s2_thresh": Case(SHAPES[2], 0.6, 256, 5422, 5356, "thresh", 5356),
    "s2_kth": Case(SHAPES[2], 0.091, 4880, 5422, 4640, "kth", 4880),
    "s2_all": Case(SHAPES[2], 0.6, 5422, 5422, 5356, "kth", 5422),
    "big_thresh": Case(BIG, 0.601, 256, 612750, 611359, "thresh", 611359),
    "big_kth": Case(BIG, 0.3, 609702, 612750, 604967, "kth", 609702),
}
SMALL = [n for n in CASES if not n.startswith("big")]
BIG_CASES = [n for n in CASES if n.startswith("big")]
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
# the (case, storage dtype) pairs the table holds for: the BIG cases in bf16 only
CASE_DTYPES = [(n, d) for n in SMALL for d in DTYPES] + [(n, torch.bfloat16) for n in BIG_CASES]


def make_inputs(shape):
    return lc.make_inputs(shape)


def make_criterion(name):
    from rgbx_semantic_segmentation_amd.utils.loss_opr import ProbOhemCrossEntropy2d
    c = CASES[name]
    return ProbOhemCrossEntropy2d(IGNORE, thresh=c.thresh, min_kept=c.min_kept)


def upsampled(lg):
    """(B, K, 4h, 4w) fp64 from low-res logits (B, h, w, K)."""
    return Fn.interpolate(lg.double().permute(0, 3, 1, 2), scale_factor=4, mode="bilinear", align_corners=False)


@functools.lru_cache(maxsize=None)
def target_prob(shape, dtype):
    """fp64 (py (B, H, W) with SENTINEL at pixels that are not valid, valid mask) on the logits rounded
    to the storage dtype."""
    lg, lab = make_inputs(shape)
    K = shape[3]
    valid = (lab != IGNORE) & (lab >= 0) & (lab < K)
    p = torch.softmax(upsampled(lg.to(dtype)), dim=1).gather(1, lab.clamp(0, K - 1).unsqueeze(1)).squeeze(1)
    return torch.where(valid, p, torch.full_like(p, SENTINEL)), valid


Expected = namedtuple("Expected", "loss dlogits gsum threshold n_valid n_below n_kept kept")


@functools.lru_cache(maxsize=None)
def expected(name, dtype):
    """The restatement in fp64 on the rounded logits: loss, d(DLOSS * loss)/d(low-res logits), the
    selection's threshold, counts and kept mask."""
    c = CASES[name]
    lg, lab = make_inputs(c.shape)
    lgr = lg.to(dtype).double()
    crit = make_criterion(name)
    ref = lc.reference_of(crit, lgr, lab)
    kept, threshold, n_valid, n_below = crit.selection(upsampled(lgr), lab)
    return Expected(ref.loss, ref.dlogits, ref.gsum, threshold, n_valid, n_below, int(kept.sum()), kept)


def host_rule(py, thresh, min_kept):
    """(threshold, n_valid, n_below, n_kept) of the select's rule on a 1-D fp32 tensor of keys, by
    sorting: a key is valid when its bit pattern is below 2.0's (0 <= key < 2); comparisons in fp32."""
    bits = py.contiguous().view(torch.int32)
    valid = (bits >= 0) & (bits < 0x40000000)
    pv = torch.sort(py[valid]).values
    n_valid, n_below = pv.numel(), int((pv <= thresh).sum())
    if min_kept <= 0 or min_kept > n_valid:
        return float("inf"), n_valid, n_below, n_valid
    if n_below >= min_kept:
        return torch.tensor(thresh, dtype=py.dtype).item(), n_valid, n_below, n_below
    kth = pv[min_kept - 1]
    return kth.item(), n_valid, n_below, int((pv <= kth).sum())


def margin_report(name, dtype):
    """The margin condition of one case on the fp64 reference: a dict of the quantities and `ok`."""
    c = CASES[name]
    py, valid = target_prob(c.shape, dtype)
    pv = torch.sort(py[valid]).values
    near = int(((pv - c.thresh).abs() < MARGIN).sum())
    if c.regime == "nofilter":
        return dict(ok=True)
    if c.regime == "thresh":
        return dict(near_thresh=near, ok=near == 0)
    k = c.min_kept
    kth = pv[k - 1].item()
    gap = (pv[k] - pv[k - 1]).item() if k < pv.numel() else float("inf")
    n_below = int((pv <= c.thresh).sum())
    return dict(kth=kth, gap=gap, near_thresh=near, n_below=n_below,
                ok=gap >= 2 * MARGIN and kth - c.thresh >= MARGIN and k - n_below > near)
