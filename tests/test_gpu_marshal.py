"""The binder's marshalling on the device: a call given tensors launches what the same call given raw
addresses and an explicit stream launches (bitwise-equal outputs), the filled stream is torch's
current stream, and a view passes its own address (nothing is copied)."""
import pytest
import torch

from rgbx_semantic_segmentation_amd import _lib
from rgbx_semantic_segmentation_amd._lib import call, dtype_code, ptr, stream

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_layernorm_fwd_tensors_equal_raw_pointers(dev, dtype):
    G, R, C = 2, 5, 32
    torch.manual_seed(0)
    x = torch.randn(G * R, C, device=dev).to(dtype)
    g, b = torch.randn(G, C, device=dev), torch.randn(G, C, device=dev)
    outs = []
    for raw in (False, True):
        y = torch.full_like(x, 7.0)
        mean, rstd = torch.full((G * R,), 7.0, device=dev), torch.full((G * R,), 7.0, device=dev)
        if raw:
            call("cmx_layernorm_fwd", ptr(x), ptr(g), ptr(b), ptr(y), ptr(mean), ptr(rstd), R, G, C, 1e-5,
                 dtype_code(x), stream())
        else:
            call("cmx_layernorm_fwd", x, g, b, y, mean, rstd, R, G, C, 1e-5, dtype_code(x))
        outs.append((y, mean, rstd))
    for a, r in zip(*outs):
        assert torch.equal(a, r)
    ref = torch.stack([torch.nn.functional.layer_norm(x.view(G, R, C)[i].float(), (C,), g[i], b[i], 1e-5)
                       for i in range(G)]).view(G * R, C)
    # the kernel ran and normalised: fp32 arithmetic, then for bf16 the store's rounding (half an ulp is
    # 2^-9 relative; 2^-7 leaves room for the fp32 differences landing on another bf16 neighbour)
    rtol, atol = (1e-5, 1e-4) if dtype == torch.float32 else (2.0 ** -7, 1e-3)
    assert torch.allclose(outs[0][0].float(), ref, rtol=rtol, atol=atol)


def test_small_linear_fwd_tensors_equal_raw_pointers(dev):
    B, Kin, Nout = 2, 40, 24
    torch.manual_seed(0)
    x, W, b = torch.randn(B, Kin, device=dev), torch.randn(Nout, Kin, device=dev), torch.randn(Nout, device=dev)
    y0, y1 = torch.full((B, Nout), 7.0, device=dev), torch.full((B, Nout), 7.0, device=dev)
    call("cmx_small_linear_fwd", x, W, b, y0, B, Kin, Nout, 0)
    call("cmx_small_linear_fwd", ptr(x), ptr(W), ptr(b), ptr(y1), B, Kin, Nout, 0, stream())
    assert torch.equal(y0, y1)
    assert (y0.double() - (x.double() @ W.double().t() + b.double())).abs().max().item() < 1e-4


def test_filled_stream_is_the_current_stream(dev, monkeypatch):
    seen = []
    monkeypatch.setattr(_lib, "observer", lambda name, fn, args: seen.append((name, args)))
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream())
    x = torch.randn(64, device=dev)
    out = torch.empty_like(x)
    with torch.cuda.stream(side):
        call("cmx_act_fwd", x, out, x.numel(), 2, 0)
    call("cmx_act_fwd", x, out, x.numel(), 2, 0)
    torch.cuda.current_stream().wait_stream(side)
    assert [n for n, _ in seen] == ["cmx_act_fwd"] * 2
    assert seen[0][1][-1] == side.cuda_stream and seen[0][1][-1] != torch.cuda.current_stream().cuda_stream
    assert seen[1][1][-1] == torch.cuda.current_stream().cuda_stream
    assert seen[0][1][:2] == (x.data_ptr(), out.data_ptr())          # the observer sees the marshalled tuple
    torch.cuda.synchronize()
    assert torch.equal(out, torch.relu(x))


def test_view_passes_its_own_address(dev, monkeypatch):
    """A strided view is not made contiguous: the kernel reads the n elements that start at the view's
    address (base[2:2 + n]), not the view's elements (base[2::2])."""
    seen = []
    monkeypatch.setattr(_lib, "observer", lambda name, fn, args: seen.append(args))
    base = torch.randn(64, device=dev)
    view = base[2::2]
    assert not view.is_contiguous()
    n = 16
    out = torch.empty(n, device=dev)
    call("cmx_act_fwd", view, out, n, 2, 0)
    assert seen[0][0] == view.data_ptr() == base.data_ptr() + 2 * base.element_size()
    assert torch.equal(out, torch.relu(base[2:2 + n]))
