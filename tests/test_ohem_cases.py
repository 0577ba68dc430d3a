"""CPU checks of ProbOhemCrossEntropy2d (no GPU): the plain-PyTorch restatement against an independent
sort-based statement, the case table's literal counts and its margin condition, which criteria the
model builder and train.py accept and refuse, and the new entry points' export and argument refusal."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ohem_cases as oc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sorted_statement(py, valid, nll, thresh, min_kept):
    """numpy on p_y: (loss, threshold, n_valid, n_below, n_kept) of the rule, written with a full sort."""
    pv = np.sort(py[valid])
    n_valid, n_below = pv.size, int((pv <= thresh).sum())
    if min_kept <= 0 or min_kept > n_valid:
        keep, threshold = valid, np.inf
    else:
        threshold = max(thresh, pv[min_kept - 1])
        keep = valid & (py <= threshold)
    return nll[keep].mean(), threshold, n_valid, n_below, int(keep.sum())


@pytest.mark.parametrize("dtype", oc.DTYPES, ids=str)
@pytest.mark.parametrize("name", oc.SMALL)
def test_restatement_equals_the_sorted_statement_and_the_table(name, dtype):
    c = oc.CASES[name]
    lg, lab = oc.make_inputs(c.shape)
    z = oc.upsampled(lg.to(dtype))
    py, valid = oc.target_prob(c.shape, dtype)
    nll = -torch.log_softmax(z, dim=1).gather(1, lab.clamp(0, c.shape[3] - 1).unsqueeze(1)).squeeze(1)
    loss, threshold, n_valid, n_below, n_kept = sorted_statement(py.numpy(), valid.numpy(), nll.numpy(), c.thresh,
                                                                 c.min_kept)
    e = oc.expected(name, dtype)
    assert (e.n_valid, e.n_below, e.n_kept) == (n_valid, n_below, n_kept) == (c.n_valid, c.n_below, c.n_kept)
    assert e.threshold == threshold and abs(e.loss.item() - loss) <= 1e-12 * abs(loss)
    regime = "nofilter" if threshold == np.inf else "thresh" if threshold == c.thresh else "kth"
    assert regime == c.regime
    assert e.dlogits.abs().max() > 0 and torch.isfinite(e.dlogits).all()


@pytest.mark.parametrize("name,dtype", oc.CASE_DTYPES, ids=lambda v: str(v))
def test_margin_condition(name, dtype):
    """No decision of a case sits within MARGIN = 5 x the kernel's p_y error bound of a tie."""
    c = oc.CASES[name]
    rep = oc.margin_report(name, dtype)
    py, valid = oc.target_prob(c.shape, dtype)
    pv = py[valid]
    assert pv.numel() == c.n_valid and int((pv <= c.thresh).sum()) == c.n_below
    assert rep["ok"], rep


def test_no_filter_is_cross_entropy_bit_for_bit():
    for name in ("s0_nofilter", "s0_minkept0"):
        c = oc.CASES[name]
        lg, lab = oc.make_inputs(c.shape)
        z = oc.upsampled(lg)
        got = oc.make_criterion(name)(z, lab)
        assert torch.equal(got, nn.CrossEntropyLoss(ignore_index=oc.IGNORE)(z, lab)) and got.dtype == torch.float64
    lab = torch.full((1, 4, 4), oc.IGNORE)
    assert torch.isnan(oc.make_criterion("s1_thresh")(torch.zeros(1, 3, 4, 4, dtype=torch.float64), lab))


def test_module_keeps_the_reference_signature():
    from rgbx_semantic_segmentation_amd.utils.loss_opr import ProbOhemCrossEntropy2d
    m = ProbOhemCrossEntropy2d(255)
    assert (m.ignore_label, m.thresh, m.min_kept, m.down_ratio, m.reduction) == (255, 0.6, 256, 1, "mean")
    assert isinstance(m.criterion, nn.CrossEntropyLoss) and m.criterion.ignore_index == 255
    m = ProbOhemCrossEntropy2d(7, "sum", 0.7, 100000, 8, False)
    assert (m.ignore_label, m.thresh, m.min_kept, m.down_ratio, m.criterion.reduction) == (7, 0.7, 100000, 8, "sum")
    with pytest.raises(NotImplementedError, match="use_weight"):
        ProbOhemCrossEntropy2d(255, use_weight=True)


def test_builder_accepts_ohem():
    from rgbx_semantic_segmentation_amd.models.builder import DiceSpec, EncoderDecoder, OhemSpec, _loss_plan
    from rgbx_semantic_segmentation_amd.utils.loss_opr import ProbOhemCrossEntropy2d
    ig, spec, w = _loss_plan(ProbOhemCrossEntropy2d(3, thresh=0.7, min_kept=1000))
    assert ig == 3 and w is None and isinstance(spec, OhemSpec) and spec == (0.7, 1000)
    assert not isinstance(spec, DiceSpec) and isinstance(spec[1], int)
    crit = oc.make_criterion("s1_kth")
    m = EncoderDecoder(dict(backbone="mit_b0", num_classes=9), criterion=crit)
    assert m.criterion is crit and m.ignore_index == oc.IGNORE and m._loss_weight is None
    assert isinstance(m._loss_spec, OhemSpec) and m._loss_spec == (0.07, 3581)
    for red in ("sum", "none"):
        with pytest.raises(NotImplementedError, match="CE_Focal"):
            _loss_plan(ProbOhemCrossEntropy2d(255, reduction=red))
    with pytest.raises(NotImplementedError, match="ProbOhemCrossEntropy2d"):
        _loss_plan(nn.MSELoss())                  # the message names the grown set


def test_train_parser_and_factory_for_ohem():
    sys.path.insert(0, ROOT)
    import train
    from rgbx_semantic_segmentation_amd.utils.loss_opr import ProbOhemCrossEntropy2d
    parse = train.build_parser().parse_args
    a = parse([])
    assert (a.ohem_thresh, a.ohem_min_kept) == (0.6, 256) and "ProbOhemCrossEntropy2d" in train.CRITERIA
    crit = train.build_criterion(parse(["--criterion", "ProbOhemCrossEntropy2d"]))
    assert isinstance(crit, ProbOhemCrossEntropy2d)
    assert (crit.ignore_label, crit.thresh, crit.min_kept, crit.reduction) == (255, 0.6, 256, "mean")
    crit = train.build_criterion(parse(["--criterion", "ProbOhemCrossEntropy2d", "--ohem-thresh", "0.7",
                                        "--ohem-min-kept", "100000"]), background=0)
    assert (crit.ignore_label, crit.thresh, crit.min_kept) == (0, 0.7, 100000)
    with pytest.raises(NotImplementedError, match="class-weights"):
        train.build_criterion(parse(["--criterion", "ProbOhemCrossEntropy2d", "--num-classes", "3",
                                     "--class-weights", "1,2,0.5"]))
    with pytest.raises(NotImplementedError, match="--dice-alpha"):
        train.build_criterion(parse(["--criterion", "ProbOhemCrossEntropy2d", "--dice-alpha", "0.5"]))
    for name in ("DiceCELoss", "BalanceLoss", "TopologyAwareCE"):
        with pytest.raises(NotImplementedError, match="FocalLoss2d"):
            train.build_criterion(parse(["--criterion", name]))


def test_ohem_entry_points_exported_and_abi_unchanged():
    """The four entry points are declared in include/cmx_ohem.h (part 2 of the library's ABI, with a
    binding table of its own), exported and callable by name; cmx_hip.h and its table are as they were."""
    from rgbx_semantic_segmentation_amd import _lib
    sigs = _lib.parse_header(os.path.join(ROOT, "include", "cmx_ohem.h"))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    names = ("cmx_ohem_select_workspace", "cmx_ohem_select", "cmx_upsample_ohem_workspace", "cmx_upsample_ohem_fwd_adj")
    assert tuple(sigs) == names == tuple(_lib.OHEM_SIGNATURES)
    for name in names:
        assert hasattr(lib, name) and name not in _lib.SIGNATURES, name
        assert _lib.OHEM_SIGNATURES[name].kinds == sigs[name].kinds
    assert [len(sigs[n][1]) for n in names] == [1, 8, 3, 18]
    assert sigs["cmx_ohem_select"].kinds == (_lib.POINTER,) + (_lib.SCALAR,) * 3 + (_lib.POINTER,) * 3 + (_lib.STREAM,)
    assert lib.cmx_abi_version() == _lib.header_abi_version() == 7
    # two counters (padded to four words) and histograms of 2048, 2048 and 1024 (padded) bins
    assert _lib.query("cmx_ohem_select_workspace", 1000) == (4 + 3 * 2048) * 4
    assert _lib.query("cmx_upsample_ohem_workspace", 2, 13, 17) == (4 + 3 * 2048) * 4 + 2 * 3 * 3 * 2 * 4
    assert _lib.query("cmx_ohem_select_workspace", 0) == _lib.query("cmx_upsample_ohem_workspace", 0, 5, 7) == 0
    with pytest.raises(TypeError, match="cmx_ohem_select"):
        _lib.marshal("cmx_ohem_select", (None, 10, 0.6))


def test_ohem_entry_points_reject_bad_arguments_without_launching():
    """K = 41 and a non-x4 size return CMX_ERR_SHAPE with a message naming the sizes before anything is
    launched (every pointer is NULL); a NaN thresh, n <= 0, null operands and an unknown dtype are
    refused too."""
    from rgbx_semantic_segmentation_amd import _lib
    fn = _lib.LIB.cmx_upsample_ohem_fwd_adj
    null = (None,) * 7
    nan = float("nan")
    st = fn(*null, 1, 2, 2, 8, 8, 41, 255, 0.6, 256, 1, None)
    assert st == _lib.CMX_ERR_SHAPE and "K=41" in _lib.last_error()
    st = fn(*null, 1, 2, 2, 8, 9, 9, 255, 0.6, 256, 1, None)
    assert st == _lib.CMX_ERR_SHAPE and "2x2 -> 8x9" in _lib.last_error()
    st = fn(*null, 1, 2, 2, 8, 8, 9, 255, nan, 256, 1, None)
    assert st == _lib.CMX_ERR_ARG and "NaN" in _lib.last_error()
    st = fn(*null, 1, 2, 2, 8, 8, 9, 255, 0.6, 256, 3, None)
    assert st == _lib.CMX_ERR_DTYPE and "dtype" in _lib.last_error()
    st = fn(*null, 1, 2, 2, 8, 8, 9, 255, 0.6, 256, 1, None)
    assert st == _lib.CMX_ERR_ARG and "null" in _lib.last_error()
    sel = _lib.LIB.cmx_ohem_select
    assert sel(None, 10, nan, 3, None, None, None, None) == _lib.CMX_ERR_ARG and "NaN" in _lib.last_error()
    assert sel(None, 0, 0.6, 3, None, None, None, None) == _lib.CMX_ERR_ARG and "n=0" in _lib.last_error()
    assert sel(None, 2 ** 31, 0.6, 3, None, None, None, None) == _lib.CMX_ERR_ARG
    assert sel(None, 10, 0.6, 3, None, None, None, None) == _lib.CMX_ERR_ARG and "null" in _lib.last_error()
