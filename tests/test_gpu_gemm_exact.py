"""Every kernel variant of the MFMA GEMM family on inputs for which the result is exact
(tests/gemm_cases.py: the case table, the input generator, the guarded buffers and the fp64
reference; tests/test_gemm_variants.py pins each case to the variant it names, on the CPU).

Every assertion on a result is torch.equal with the fp64 reference cast to the stored type --
fp32 store / accumulate: `ref.float()`; 16-bit store: `ref.float().to(dtype)`, the hardware's
round-to-nearest-even -- after the helper has checked, on the reference alone, that the reference
is exactly representable in fp32.  The one tolerance is GELU's: |y - ref| <= delta(v) + u |ref|
against fp64 erf-GELU of the exact pre-activation v, delta derived in gemm_cases.py (gelu_delta)
from the pinned erf bound and the fp32 roundings around it, u = 2^-8 (bf16) / 2^-11 (fp16) / 0.
Around every case: sentinel guard columns and rows around C, R and the mask that must survive,
and NaN padding after column K and after the last row of A and B."""
import contextlib
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_cases as gc  # noqa: E402

pytestmark = pytest.mark.gpu
RUNS = gc.runs()


def _dtype(name):
    return getattr(torch, name)


def _need_256_cus():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cus != gc.NUM_CU:
        pytest.skip(f"the case's plan is pinned at {gc.NUM_CU} CUs, this device reports {cus}")


@contextlib.contextmanager
def tuned(knobs):
    """the case's knob overrides for the launches inside; the values read before are restored"""
    from rgbx_semantic_segmentation_amd import kernels as Kn
    old = {}
    if knobs:
        a = torch.ones(1, 8, 8, device="cuda", dtype=torch.bfloat16)
        Kn.gemm(a, a, torch.empty(1, 8, 8, device="cuda", dtype=torch.bfloat16))   # (registers the knobs)
    try:
        for k, v in knobs.items():
            old[k] = Kn.tune_get(k)
            assert old[k] == gc.KNOB_DEFAULTS[k], f"{k} = {old[k]} before the test: the plans assume the defaults"
            Kn.tune(k, v)
        yield
    finally:
        for k, v in old.items():
            Kn.tune(k, v)


@pytest.mark.parametrize("run", RUNS, ids=[gc.run_id(r) for r in RUNS])
def test_gemm_exact(dev, run):
    from rgbx_semantic_segmentation_amd import kernels as Kn
    c = run.case
    if c.cu:
        _need_256_cus()
    p = gc.Problem(c.G, c.M, c.N, c.K, c.tA, c.tB, run.epi, _dtype(run.dtype), dev, cvec=c.cvec)
    ones = int("dbias" in p.kw)
    if run.dtype != "float32":
        # the launch takes the path the variant was planned for ...
        assert gc.fast_ok(p.kw["A"], p.kw.get("A2"), p.kw["B"], c.M, c.N + ones, c.K, c.tA, c.tB, ones) == bool(c.fast)
    with tuned(c.knobs):
        # ... and the split the wrapper asks the library for is the planned one
        if c.splitk <= 0:
            sk = Kn.query("cmx_gemm_splitk", c.G, c.M, c.N + ones, c.K, ones, gc.DTYPE_CODE[run.dtype])
            assert (sk > 1) == run.variant.split, sk
        Kn.gemm(splitk=c.splitk, **p.kw)
    torch.cuda.synchronize()
    p.check(gc.run_id(run))


def test_gemm_ln_stored_output_exact(dev):
    """cmx_gemm_ln is the one launch on 64 x 128 NS4 tiles: the C it stores (bias, DropPath-scaled
    residual), exactly; the normalised output is test_gemm_ln_tail's."""
    from rgbx_semantic_segmentation_amd import kernels as Kn
    c = gc.LN_CASE
    for name in c.dtypes:
        p = gc.Problem(c.G, c.M, c.N, c.K, 0, 0, c.epis[0], _dtype(name), dev, contiguous=True)
        kw = dict(p.kw)
        assert kw.pop("out_mode") == 0 and kw.pop("act") == "none" and p.C.is_contiguous()
        gamma = torch.ones(c.G, c.N, device=dev)
        out = Kn.gemm_ln(kw.pop("A"), kw.pop("B"), kw.pop("C"), gamma, torch.zeros_like(gamma), 1e-6, **kw)
        assert out is not None, "gemm_ln refused an eligible problem"
        torch.cuda.synchronize()
        p.check(f"{c.name}-{name}")
        assert bool(torch.isfinite(out[0].float()).all())


@pytest.mark.parametrize("mc", gc.MULTI_CASES, ids=[m.name for m in gc.MULTI_CASES])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_gemm_multi_exact(dev, mc, dtype):
    """2-3 problems as one cmx_gemm_multi grid (functions._gemm_group), each checked exactly"""
    from rgbx_semantic_segmentation_amd import functions as Fn
    from rgbx_semantic_segmentation_amd import kernels as Kn
    assert Fn.MULTI_GEMM
    probs = []
    for G, M, N, K, epi in mc.problems:
        probs.append(gc.Problem(G, M, N, K, 0, mc.tB, epi, dtype, dev))
    jobs = [p.kw for p in probs]
    assert all(Kn.gemm(plan=True, **j) is not None for j in jobs), "a problem is not eligible for the multi launch"
    Fn._gemm_group(jobs)
    torch.cuda.synchronize()
    for i, p in enumerate(probs):
        p.check(f"{mc.name}[{i}]-{dtype}")
