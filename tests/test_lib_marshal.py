"""The binder's argument marshalling (_lib.marshal), on the host: parameter kinds come from the
header, tensors become addresses in pointer slots only, a left-out trailing stream is filled, and a
wrong argument count is a TypeError instead of ctypes' silent acceptance.  Nothing is launched: every
call here either stops in marshal or is refused by the entry point's host-side validation."""
import ctypes

import pytest
import torch

from rgbx_semantic_segmentation_amd import _lib
from rgbx_semantic_segmentation_amd._lib import POINTER, SCALAR, STREAM


def _ln_args(C=32, dtype=torch.float32):
    x = torch.zeros(10, C, dtype=dtype)
    return x, torch.ones(1, C), torch.zeros(1, C), torch.empty_like(x)


def test_header_kinds():
    sigs = _lib.SIGNATURES
    assert len(sigs) == 130
    for name, sig in sigs.items():
        rt, argt = sig
        assert len(sig.kinds) == len(argt), name
        assert set(sig.kinds) <= {POINTER, STREAM, SCALAR}, name
        assert STREAM not in sig.kinds[:-1], name
        for kind, ct in zip(sig.kinds, argt):
            if kind != SCALAR:
                assert ct is ctypes.c_void_p, (name, kind, ct)
    assert sum(1 for s in sigs.values() if s.kinds[-1:] == (STREAM,)) == 90
    assert sigs["cmx_tune"].kinds == (SCALAR, SCALAR)                      # const char* is no pointer slot
    assert sigs["cmx_layernorm_fwd"].kinds == (POINTER,) * 6 + (SCALAR,) * 5 + (STREAM,)
    assert _lib.parse_header()["cmx_layernorm_fwd"].kinds == sigs["cmx_layernorm_fwd"].kinds


def test_marshal_pointer_and_scalar_slots():
    x, g, b, y = _ln_args()
    m = _lib.marshal("cmx_layernorm_fwd", (x, g, b, y[1:], None, 12345, 10, True, 32, 1e-5, 0, 0))
    assert m[:4] == (x.data_ptr(), g.data_ptr(), b.data_ptr(), y.data_ptr() + y.stride(0) * y.element_size())
    assert m[4] is None                                  # NULL
    assert m[5] == 12345 and type(m[5]) is int           # an integer address passes through
    assert m[7] == 1 and type(m[7]) is int               # bool -> int
    assert m[6:] == (10, 1, 32, 1e-5, 0, 0)
    t = torch.zeros(8)
    assert _lib.marshal("cmx_cast_f32_bf16", (t[1:], t, 4, 0))[0] == t.data_ptr() + t.element_size()


def test_missing_trailing_stream_is_filled(monkeypatch):
    monkeypatch.setattr(_lib, "stream", lambda: 0xABCD)
    x, g, b, y = _ln_args()
    m = _lib.marshal("cmx_layernorm_fwd", (x, g, b, y, None, None, 10, 1, 32, 1e-5, 0))
    assert len(m) == 12 and m[-1] == 0xABCD
    m = _lib.marshal("cmx_layernorm_fwd", (x, g, b, y, None, None, 10, 1, 32, 1e-5, 0, 7))
    assert m[-1] == 7                                    # an explicit stream is kept
    # no stream parameter: nothing is filled, the count must match
    assert _lib.marshal("cmx_tune_get", (b"GEMM_SMALLK",)) == (b"GEMM_SMALLK",)
    with pytest.raises(TypeError, match="cmx_tune_get"):
        _lib.marshal("cmx_tune_get", ())


def test_wrong_counts_and_kinds_raise():
    x, g, b, y = _ln_args()
    full = (x, g, b, y, None, None, 10, 1, 32, 1e-5, 0, 0)
    with pytest.raises(TypeError, match=r"cmx_layernorm_fwd takes 12 arguments, 13 given"):
        _lib.call("cmx_layernorm_fwd", *full, 0)
    with pytest.raises(TypeError, match=r"cmx_layernorm_fwd takes 12 arguments, 10 given"):
        _lib.try_call("cmx_layernorm_fwd", *full[:10])
    with pytest.raises(TypeError, match="cmx_tune_get"):
        _lib.query("cmx_tune_get", b"NOPE", 1, 2)        # ctypes alone accepts the surplus arguments
    with pytest.raises(TypeError, match="scalar"):
        _lib.marshal("cmx_layernorm_fwd", (x, g, b, y, None, None, torch.tensor(10), 1, 32, 1e-5, 0, 0))


def test_refusal_arrives_through_call():
    """C = 30 is refused by cmx_layernorm_fwd's host-side validation, before any launch."""
    x, g, b, y = _ln_args(C=30)
    with pytest.raises(_lib.CMXError, match="layernorm_fwd"):
        _lib.call("cmx_layernorm_fwd", x, g, b, y, None, None, 10, 1, 30, 1e-5, 1, 0)
    assert _lib.try_call("cmx_layernorm_fwd", x, g, b, y, None, None, 10, 1, 30, 1e-5, 1, 0) == _lib.CMX_ERR_SHAPE


def test_refusable_returns_sentinel_for_named_codes_only():
    x, g, b, y = _ln_args(C=30)
    args = (x, g, b, y, None, None, 10, 1, 30, 1e-5, 1, 0)
    assert _lib.refusable("cmx_layernorm_fwd", (_lib.CMX_ERR_SHAPE,), *args) is _lib.REFUSED
    assert _lib.refusable("cmx_layernorm_fwd", (_lib.CMX_ERR_ARG, _lib.CMX_ERR_SHAPE), *args) is _lib.REFUSED
    with pytest.raises(_lib.CMXError, match="layernorm_fwd"):
        _lib.refusable("cmx_layernorm_fwd", (_lib.CMX_ERR_ARG,), *args)


def test_one_dtype_table():
    from rgbx_semantic_segmentation_amd import deferred, kernels
    assert _lib.DTYPE_CODES == {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
    for dt, code in _lib.DTYPE_CODES.items():
        assert _lib.dtype_code(torch.empty(1, dtype=dt)) == code
    with pytest.raises(_lib.CMXError):
        _lib.dtype_code(torch.empty(1, dtype=torch.float64))
    assert deferred._operand is kernels._operand
