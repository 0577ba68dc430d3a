"""CPU checks of the loss family (no GPU): the closed-form gradients the kernels implement against
fp64 autograd of the plain-PyTorch restatement, the uniform closed form, which criteria the model
builder and train.py accept and refuse, and the new entry points' export and shape refusal."""
import ctypes
import os
import sys

import pytest
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_cases as lc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _full_res(K, seed=0):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(2, K, 9, 11, dtype=torch.float64, generator=g) * 3
    lab = torch.randint(0, K, (2, 9, 11), generator=g)
    lab[:, 2:5, 3:8] = lc.IGNORE
    return z, lab


@pytest.mark.parametrize("gamma", [0.0, 1.0, 2.0, 4.0, 2.5])
def test_focal_gradient_formula_matches_autograd(gamma):
    """u_k = dl/dp_k, dl/dz_j = p_j (u_j - sum_k u_k p_k): < 1e-12 relative against fp64 autograd."""
    from rgbx_semantic_segmentation_amd.utils.loss_opr import FocalLoss, focal_grad
    z, lab = _full_res(7)
    lab[0, 0, 0] = 7 + 3                          # clamped to class 6, and valid
    crit = FocalLoss(lc.IGNORE, gamma=gamma, alpha=lc.ALPHA)
    zr = z.clone().requires_grad_(True)
    crit.pixel_loss(zr, lab)[0].sum().backward()
    g = focal_grad(z, lab, lc.IGNORE, gamma, lc.ALPHA)
    assert lc.relerr(g, zr.grad) < 1e-12
    assert g[:, :, 2:5, 3:8].abs().max() == 0 and g[0, :, 0, 0].abs().max() > 0


@pytest.mark.parametrize("weighted", [False, True])
def test_focal2d_gradient_formula_matches_autograd(weighted):
    """c (p - onehot), c = w_y ((1 - p)^2 - 2 p (1 - p) log p), against fp64 autograd of the
    un-normalised NLLLoss((1 - p)^2 log p)."""
    from rgbx_semantic_segmentation_amd.utils.loss_opr import FocalLoss2d, focal2d_grad
    K = 7
    z, lab = _full_res(K, seed=1)
    w = lc.class_weights(K).double() if weighted else None
    crit = FocalLoss2d(weight=None if w is None else w.tolist(), reduction="sum", ignore_index=lc.IGNORE)
    zr = z.clone().requires_grad_(True)
    lc.Restated(crit)(zr, lab).backward()
    assert lc.relerr(focal2d_grad(z, lab, lc.IGNORE, w), zr.grad) < 1e-12


def test_focal2d_ignores_its_gamma():
    from rgbx_semantic_segmentation_amd.utils.loss_opr import FocalLoss2d
    z, lab = _full_res(5, seed=2)
    assert torch.equal(FocalLoss2d(gamma=0)(z, lab), FocalLoss2d(gamma=3)(z, lab))


@pytest.mark.parametrize("gamma", [0.0, 4.0])
def test_uniform_closed_form_fp64(gamma):
    """All-zero logits: every p_k = 1/K; the restatement gives the closed form per valid pixel,
    and nothing valid gives 0 (not NaN)."""
    from rgbx_semantic_segmentation_amd.utils.loss_opr import FocalLoss
    K = 9
    crit = FocalLoss(lc.IGNORE, gamma=gamma, alpha=lc.ALPHA)
    lg, lab = lc.make_inputs((1, 15, 20, K), kind="uniform")
    ref = lc.reference_of(crit, lg, lab)
    n = int((lab != lc.IGNORE).sum())                 # the mean divides by n + 1e-8
    want = lc.uniform_focal_loss(K, gamma) * n / (n + 1e-8)
    assert abs(ref.loss.item() - want) < 1e-12 * want
    lg, lab = lc.make_inputs((1, 15, 20, K), ignored="all")
    ref = lc.reference_of(crit, lg, lab)
    assert ref.loss.item() == 0.0 and ref.dlogits.abs().max() == 0


def test_builder_accepts_the_four_criteria_and_refuses_the_rest():
    from rgbx_semantic_segmentation_amd import functions as F
    from rgbx_semantic_segmentation_amd.models.builder import EncoderDecoder
    from rgbx_semantic_segmentation_amd.utils.loss_opr import FocalLoss, FocalLoss2d
    cfg = dict(backbone="mit_b0", num_classes=9)
    assert EncoderDecoder(cfg)._loss_spec is None
    for name, kind, ce_scale, focal_scale in [("focal_g4", F.LOSS_FOCAL, 0.0, 1.0), ("ce_focal", F.LOSS_FOCAL, 1.0, 0.2),
                                              ("wce", F.LOSS_WCE, 1.0, 0.0), ("fl2d", F.LOSS_FOCAL2D, 1.0, 0.0),
                                              ("fl2d_w", F.LOSS_FOCAL2D, 1.0, 0.0)]:
        crit = lc.make_criterion(name, 9)
        m = EncoderDecoder(cfg, criterion=crit)
        assert m.criterion is crit and m.ignore_index == lc.IGNORE
        assert m._loss_spec[0] == kind and m._loss_spec[3:] == (ce_scale, focal_scale), name
        assert (m._loss_weight is not None) == (name in ("wce", "fl2d_w"))
    assert EncoderDecoder(cfg, criterion=lc.make_criterion("focal_g4", 9))._loss_spec[1:3] == (4.0, lc.ALPHA)
    ce = nn.CrossEntropyLoss
    for bad in [ce(label_smoothing=0.1), ce(reduction="sum"), FocalLoss(255, reduction="sum"),
                FocalLoss2d(reduction="none"), nn.MSELoss(), "DiceLoss", (ce(), ce()),
                (ce(weight=torch.ones(9)), FocalLoss(255)), (ce(ignore_index=0), FocalLoss(255))]:
        with pytest.raises(NotImplementedError, match="CE_Focal"):
            EncoderDecoder(cfg, criterion=bad)
    for gamma in (0.5, -1.0):
        with pytest.raises(ValueError, match="gamma"):
            EncoderDecoder(cfg, criterion=FocalLoss(255, gamma=gamma))
        with pytest.raises(ValueError, match="gamma"):
            EncoderDecoder(cfg, criterion=(ce(ignore_index=255), FocalLoss(255, gamma=gamma)))


def test_train_parser_and_criterion_factory():
    sys.path.insert(0, ROOT)
    import train
    from rgbx_semantic_segmentation_amd.utils.loss_opr import FocalLoss, FocalLoss2d
    a = train.build_parser().parse_args([])
    assert (a.criterion, a.fl_gamma, a.fl_alpha, a.class_weights) == ("CrossEntropyLoss", 4.0, 0.25, "")
    assert isinstance(train.build_criterion(a), nn.CrossEntropyLoss)
    a = train.build_parser().parse_args(["--criterion", "CE_Focal", "--fl-gamma", "2", "--fl-alpha", "0.5"])
    ce, fl = train.build_criterion(a)
    assert isinstance(ce, nn.CrossEntropyLoss) and isinstance(fl, FocalLoss) and (fl.gamma, fl.alpha) == (2.0, 0.5)
    assert fl.ignore_label == ce.ignore_index == 255
    a = train.build_parser().parse_args(["--criterion", "FocalLoss"])
    assert train.build_criterion(a).gamma == 4.0
    a = train.build_parser().parse_args(["--criterion", "FocalLoss2d", "--num-classes", "3", "--class-weights", "1,2,0.5"])
    crit = train.build_criterion(a)
    assert isinstance(crit, FocalLoss2d) and crit.loss.weight.tolist() == [1.0, 2.0, 0.5]
    a = train.build_parser().parse_args(["--num-classes", "3", "--class-weights", "1,2,0.5"])
    assert train.build_criterion(a).weight.tolist() == [1.0, 2.0, 0.5]
    with pytest.raises(ValueError):
        train.build_criterion(train.build_parser().parse_args(["--class-weights", "1,2"]))
    for name in ("DiceCELoss", "BalanceLoss", "TopologyAwareCE"):
        with pytest.raises(NotImplementedError, match="FocalLoss2d"):
            train.build_criterion(train.build_parser().parse_args(["--criterion", name]))


def test_loss_entry_points_exported_and_abi_unchanged():
    from rgbx_semantic_segmentation_amd import _lib
    sigs = _lib.parse_header(os.path.join(ROOT, "include", "cmx_hip.h"))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("cmx_upsample_loss_fwd_adj", "cmx_upsample_loss_workspace"):
        assert name in sigs and hasattr(lib, name), name
    assert len(sigs["cmx_upsample_loss_fwd_adj"][1]) == 20
    assert lib.cmx_abi_version() == _lib.header_abi_version() == 7
    # per-block [loss, normaliser] partials of the 6 x 8 low-res tiling
    assert _lib.query("cmx_upsample_loss_workspace", 2, 13, 17) == 2 * 3 * 3 * 2 * 4


def test_loss_entry_point_rejects_bad_shapes_without_launching():
    """K = 41 and a non-x4 size return CMX_ERR_SHAPE with a message before anything is launched
    (every pointer is NULL); a gamma in (0, 1) and an unknown kind are argument errors."""
    from rgbx_semantic_segmentation_amd import _lib
    fn = _lib.LIB.cmx_upsample_loss_fwd_adj
    tail = (255, 2, 4.0, 0.25, 0.0, 1.0, 1, None)
    st = fn(None, None, None, None, None, None, 1, 2, 2, 8, 8, 41, *tail)
    assert st == -1 and "K=41" in _lib.last_error()
    st = fn(None, None, None, None, None, None, 1, 2, 2, 8, 9, 9, *tail)
    assert st == -1 and "2x2 -> 8x9" in _lib.last_error()
    st = fn(None, None, None, None, None, None, 1, 2, 2, 8, 8, 9, 255, 2, 0.5, 0.25, 0.0, 1.0, 1, None)
    assert st == -4 and "gamma" in _lib.last_error()
    st = fn(None, None, None, None, None, None, 1, 2, 2, 8, 8, 9, 255, 3, 4.0, 0.25, 0.0, 1.0, 1, None)
    assert st == -4 and "kind" in _lib.last_error()
