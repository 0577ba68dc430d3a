"""CPU-only checks of the SGD-with-momentum path (``--optimizer SGDM``): the C-ABI declares and
exports ``cmx_sgdm_step`` without a revision bump, its argument refusals precede any launch,
``train.py`` parses and checks the optimizer switch, and ``FusedSGD`` refuses what
``torch.optim.SGD`` refuses (and what the kernel does not implement) before it touches a model."""
import ctypes
import os
import sys
from types import SimpleNamespace

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def test_header_declares_and_library_exports_sgdm_step():
    from rgbx_semantic_segmentation_amd import _lib
    sigs = _lib.parse_header(os.path.join(ROOT, "include", "cmx_hip.h"))
    assert "cmx_sgdm_step" in sigs
    rt, argt = sigs["cmx_sgdm_step"]
    assert rt is ctypes.c_int32 and len(argt) == 16
    assert argt[6] is ctypes.c_int64 and argt[8] is ctypes.c_double and argt[9] is ctypes.c_double
    assert argt[11] is ctypes.c_float and argt[14] is ctypes.c_int32
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "cmx_sgdm_step")
    assert lib.cmx_abi_version() == _lib.header_abi_version() == 7      # a pure addition


def test_train_parses_sgdm_and_momentum():
    import train
    p = train.build_parser()
    a = p.parse_args(["--optimizer", "SGDM"])
    assert a.optimizer == "SGDM" and a.momentum == 0.9
    assert p.parse_args([]).optimizer == "AdamW"
    assert p.parse_args(["--momentum", "0.5"]).momentum == 0.5
    assert train.OPTIMIZERS == ("AdamW", "SGDM")


def test_check_optimizer():
    import train
    for name in ("AdamW", "SGDM"):
        train.check_optimizer(SimpleNamespace(optimizer=name))
    for name in ("LBFGS", "sgdm", "Adam"):
        with pytest.raises(NotImplementedError, match="SGDM"):
            train.check_optimizer(SimpleNamespace(optimizer=name))


class _NoStore:
    """A model whose store must not be reached: the hyperparameter checks come first."""

    @property
    def store(self):
        raise AssertionError("FusedSGD touched model.store before checking its hyperparameters")


@pytest.mark.parametrize("kwargs, exc, match", [
    (dict(lr=-1e-3), ValueError, "Invalid learning rate"),
    (dict(lr=1e-2, momentum=-0.1), ValueError, "Invalid momentum value"),
    (dict(lr=1e-2, weight_decay=-0.01), ValueError, "Invalid weight_decay value"),
    (dict(lr=1e-2, nesterov=True), ValueError, "Nesterov momentum requires a momentum and zero dampening"),
    (dict(lr=1e-2, momentum=0.9, dampening=0.1, nesterov=True), ValueError,
     "Nesterov momentum requires a momentum and zero dampening"),
    (dict(lr=1e-2, momentum=0.9, dampening=0.1), NotImplementedError, "dampening"),
    (dict(lr=1e-2, momentum=0.9, maximize=True), NotImplementedError, "maximize"),
])
def test_fused_sgd_hyperparameter_errors(kwargs, exc, match):
    from rgbx_semantic_segmentation_amd.optim import FusedSGD
    with pytest.raises(exc, match=match):
        FusedSGD(_NoStore(), **kwargs)


def test_fused_sgd_errors_are_torchs():
    """The ValueErrors carry torch.optim.SGD's own messages."""
    import torch
    from rgbx_semantic_segmentation_amd.optim import FusedSGD
    w = [torch.nn.Parameter(torch.zeros(1))]
    for kwargs in (dict(lr=-1e-3), dict(lr=1e-2, momentum=-0.1), dict(lr=1e-2, weight_decay=-0.01),
                   dict(lr=1e-2, nesterov=True), dict(lr=1e-2, momentum=0.9, dampening=0.1, nesterov=True)):
        with pytest.raises(ValueError) as et:
            torch.optim.SGD(w, **kwargs)
        with pytest.raises(ValueError) as eg:
            FusedSGD(_NoStore(), **kwargs)
        assert str(eg.value) == str(et.value)


# fake non-null pointers: only ever handed to calls that validation refuses, so never dereferenced
_P, _G, _B, _S, _D, _LR = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000


@pytest.mark.parametrize("what, args, status", [
    ("n = 63", (_P, _G, _B, None, 0, _D, 63, _LR, 0.9, 0.01, 0, 1.0, None, None, 0, None), "shape"),
    ("buf NULL, momentum 0.9", (_P, _G, None, None, 0, _D, 64, _LR, 0.9, 0.01, 0, 1.0, None, None, 0, None), "arg"),
    ("buf given, momentum 0", (_P, _G, _B, None, 0, _D, 64, _LR, 0.0, 0.01, 0, 1.0, None, None, 0, None), "arg"),
    ("nesterov, momentum 0", (_P, _G, None, None, 0, _D, 64, _LR, 0.0, 0.01, 1, 1.0, None, None, 0, None), "arg"),
    ("shadow, dtype 0", (_P, _G, _B, _S, 0, _D, 64, _LR, 0.9, 0.01, 0, 1.0, None, None, 0, None), "arg"),
])
def test_sgdm_step_refuses_before_launching(what, args, status):
    from rgbx_semantic_segmentation_amd import _lib
    want = {"shape": _lib.CMX_ERR_SHAPE, "arg": _lib.CMX_ERR_ARG}[status]
    st = _lib.LIB.cmx_sgdm_step(*args)
    assert st == want, (what, st, _lib.last_error())
    assert "sgdm" in _lib.last_error()
