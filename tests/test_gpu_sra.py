"""Every kernel variant of the SRA attention family (csrc/sra_attention.hip, csrc/sra_fast.hip)
against fp64 references (tests/sra_cases.py: the case table, the input kinds, the references and
the emulated yardstick; tests/test_sra_cases.py checks the constructions on the CPU).

Every case first asserts, through kernels.sra_plan, that the launch code takes the variant the case
is meant for, under a knob context that sets every SRA knob (defaults plus the case's overrides)
and restores what it found.  Then:
  random / peaked  o within one output ulp of max |ref| (2^-8 bf16, 2^-11 fp16, 1e-4 fp32), lse
                   within 1e-4 of max |lse|, dq / dk / dv each within 2 E_emul + one ulp of max |ref|
                   (E_emul: the fp32 emulation of a 16-bit flash backward, sra_cases.emulate).
  selector         exact: o == v[t] bit for bit, |lse - 256| <= 256 * 2^-20 (the m * sl2 and * ln 2
                   roundings), dq == dk == 0, dv bit-equal to the rounded fp64 scatter-sum.  General
                   path (fp32): 1e-4 of max |expected|.
  uniform          |lse - ln Nk| <= 2e-5 (a phantom key moves it by >= 9.8e-4), o within one ulp,
                   the backward as for random.
  both dQ forms    where a case runs sra_dq_small_seq and sra_dq_small, their dq is bit-equal.
  containment      every tensor inside a larger buffer (320 rows of padding either side, row strides
                   C + 8 / 2C + 8, NaN around the inputs, a sentinel around the outputs): nothing
                   outside the logical tensors changes, the inputs are unchanged, the results are
                   finite and bit-equal to the packed-stride run.
  refusals         a stride that is no multiple of 8 and D = 48 raise CMXError and write nothing."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sra_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu


knobs, assert_plan = sc.knobs, sc.assert_plan


def run_packed(K, case, x, dtype, dev):
    """forward and backward through the tensor-level wrappers on packed tensors"""
    Bt, N, Nk, heads, D, C = case.Bt, case.N, case.Nk, case.heads, case.D, case.C
    q, kv, do = x.q.to(dev, dtype), x.kv.to(dev, dtype).contiguous(), x.do.to(dev, dtype)
    o, lse = K.sra_attn_fwd(q, kv, kv[..., C:], Bt, N, Nk, heads, D, D ** -0.5, C, 2 * C)
    dq, dkv = K.sra_attn_bwd(q, kv, kv[..., C:], o, do, lse, Bt, N, Nk, heads, D, D ** -0.5, C, 2 * C)
    torch.cuda.synchronize()
    return sc.Result(o, lse, dq, dkv)


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def check(case, kind, dtype, exp, got, tag):
    """the assertions of one run; prints every figure before it asserts"""
    C, ulp = case.C, sc.ULP[dtype]
    ref, x = exp.ref, exp.x
    msg = f"{case.name} {str(dtype)[6:]} {kind} {tag}"
    for t in got:
        assert torch.isfinite(t).all(), msg
    o, lse = got.o.double().cpu(), got.lse.double().cpu()
    gg = sc.grads(sc.Result(None, None, got.dq.double().cpu(), got.dkv.double().cpu()), C)
    if kind == "selector":
        want = sc.selector_expected(case, x, dtype)
        gw = sc.grads(want, C)
        lse_err = (lse - want.lse).abs().max().item()
        print(f"[sra] {msg}: |lse - {want.lse.flatten()[0].item():.4f}| {lse_err:.3e} "
              f"o err {(o - want.o).abs().max().item():.3e} |dq| {gg['dq'].abs().max().item():.3e} "
              f"|dk| {gg['dk'].abs().max().item():.3e} dv err {(gg['dv'] - gw['dv']).abs().max().item():.3e}")
        if dtype == torch.float32:
            # general path: fp32 exp / log of scores up to 2048 D^-1/2, not exact: the fp32 tolerance
            assert sc.relerr(o, want.o) <= 1e-4 and lse_err <= 1e-4 * want.lse.abs().max().item(), msg
            scale = max(x.do.abs().max().item() * x.kv.abs().max().item(), 1.0)
            assert gg["dq"].abs().max().item() <= 1e-4 * scale and gg["dk"].abs().max().item() <= 1e-4 * scale, msg
            assert sc.relerr(gg["dv"], gw["dv"]) <= 1e-4, msg
            return
        assert torch.equal(o, want.o), msg
        assert lse_err <= 256 * 2.0 ** -20, msg
        assert (gg["dq"] == 0).all() and (gg["dk"] == 0).all(), msg
        assert torch.equal(gg["dv"], gw["dv"]), msg
        return
    gr = sc.grads(ref, C)
    o_err = sc.relerr(o, ref.o)
    if kind == "uniform":
        lse_err, lse_tol = (lse - sc.uniform_lse(case.Nk)).abs().max().item(), 2e-5
    else:
        lse_err, lse_tol = (lse - ref.lse).abs().max().item(), 1e-4 * ref.lse.abs().max().item()
    errs = {n: sc.relerr(gg[n], gr[n]) for n in gr}
    print(f"[sra] {msg}: o {o_err:.2e} (ulp {ulp:.2e}) lse {lse_err:.2e} (tol {lse_tol:.2e}) " +
          " ".join(f"{n} {errs[n]:.2e} (E_emul {exp.e_emul[n]:.2e})" for n in errs))
    assert o_err <= ulp, msg
    assert lse_err <= lse_tol, msg
    for n in errs:
        assert errs[n] <= sc.bwd_bound(exp.e_emul[n], dtype), (msg, n, errs[n], exp.e_emul[n])


def run_case(K, case, kind, dtype, dev):
    exp = sc.expected(case, kind, dtype)
    with knobs(**case.knobs):
        if case.both_dq:
            outs = []
            for seq in (1, 0):
                K.tune("SRA_DQ_SEQ", seq)
                assert_plan(K, case, dtype, dq_seq=bool(seq))
                outs.append(run_packed(K, case, exp.x, dtype, dev))
                check(case, kind, dtype, exp, outs[-1], f"dq_seq={seq}")
            # sra_dq_small_seq keeps sra_dq_small's MFMA order per output element: the same bits
            assert torch.equal(bits(outs[0].dq), bits(outs[1].dq)), f"{case.name} {kind}: dq of dq_seq=1 and 0 differ"
            return outs[0]
        assert_plan(K, case, dtype)
        got = run_packed(K, case, exp.x, dtype, dev)
    check(case, kind, dtype, exp, got, "")
    return got


MATRIX_RUNS = sc.runs(sc.MATRIX)


@pytest.mark.parametrize("run", MATRIX_RUNS, ids=[sc.run_id(r) for r in MATRIX_RUNS])
def test_sra_variant(dev, run):
    """the variant matrix: six (QW, NW) fast forward / dQ instantiations at one and three key chunks,
    the fast dK / dV in its direct and slab forms (4, 10 and the capped 64 chunks), the three small
    kernels with both dQ forms, and the general kernels"""
    from rgbx_semantic_segmentation_amd import kernels as K
    case, dtype, kind = run
    run_case(K, case, kind, dtype, dev)


THRESHOLD_RUNS = sc.runs(sc.THRESHOLDS)


@pytest.mark.parametrize("run", THRESHOLD_RUNS, ids=[sc.run_id(r) for r in THRESHOLD_RUNS])
def test_sra_thresholds(dev, run):
    """default knobs on both sides of Nk = 320 | 321, N = 600 | 601 and N = 2048 | 2049: the plan
    changes exactly there and both sides compute the same thing"""
    from rgbx_semantic_segmentation_amd import kernels as K
    case, dtype, kind = run
    assert not case.knobs
    run_case(K, case, kind, dtype, dev)


@pytest.mark.parametrize("pin", sc.B2_PINS, ids=[p[0] for p in sc.B2_PINS])
def test_sra_plan_b2_480x640(dev, pin):
    """the launch plan of the four SRA stages of B2 at 480 x 640, bs = 2, as derived today at 256 CUs
    (no kernel is launched)"""
    from rgbx_semantic_segmentation_amd import kernels as K
    _, (Bt, N, Nk, heads), want = pin
    with knobs():
        for dtype in sc.H16:
            plan = K.sra_plan(Bt, N, Nk, heads, 64, dtype)
            if plan.cus != sc.NUM_CU:
                pytest.skip(f"the plans are pinned at {sc.NUM_CU} CUs, this device reports {plan.cus}")
            got = {k: getattr(plan, k) for k in want}
            assert got == want, plan


# --------------------------------------------------------------------------------- containment
class Guarded:
    """a (Bt, R, W) tensor as rows of stride ld inside a buffer with sc.PAD_ROWS rows before and after;
    everything outside the logical tensor holds `fill`"""

    def __init__(self, shape, ld, dtype, fill, dev, data=None, strided=True):
        Bt, R, W = shape
        rows = Bt * R
        buf = torch.full((2 * sc.PAD_ROWS + rows, ld), fill, dtype=dtype)
        inside = torch.zeros(buf.shape, dtype=torch.bool)
        inside[sc.PAD_ROWS:sc.PAD_ROWS + rows, :W] = True
        if data is not None:
            buf[sc.PAD_ROWS:sc.PAD_ROWS + rows, :W] = data.reshape(rows, W).to(dtype)
        self.inside, self.before = inside, bits(buf).clone()
        self.buf = buf.to(dev)
        self.view = self.buf[sc.PAD_ROWS:sc.PAD_ROWS + rows].view(Bt, R, ld)[..., :W]
        assert self.view.data_ptr() % 16 == 0 and (ld % 8 == 0 or not strided)

    def after(self):
        return bits(self.buf.cpu())

    def unchanged(self):
        return torch.equal(self.after(), self.before)

    def outside_unchanged(self):
        return torch.equal(self.after()[~self.inside], self.before[~self.inside])

    def packed(self):
        return self.view.contiguous()


def run_guarded(K, case, x, dtype, dev):
    """forward and backward through the C-ABI with every tensor guarded and strided"""
    Bt, N, Nk, heads, D, C = case.Bt, case.N, case.Nk, case.heads, case.D, case.C
    nan, code, scale = float("nan"), K.dtype_code(torch.empty(0, dtype=dtype)), float(D ** -0.5)
    q = Guarded((Bt, N, C), C + 8, dtype, nan, dev, x.q)
    kv = Guarded((Bt, Nk, 2 * C), 2 * C + 8, dtype, nan, dev, x.kv)
    do = Guarded((Bt, N, C), C + 8, dtype, nan, dev, x.do)
    o = Guarded((Bt, N, C), C + 8, dtype, sc.SENTINEL, dev)
    dq = Guarded((Bt, N, C), C + 8, dtype, sc.SENTINEL, dev)
    dkv = Guarded((Bt, Nk, 2 * C), 2 * C + 8, dtype, sc.SENTINEL, dev)
    lse = Guarded((1, 1, Bt * heads * N), Bt * heads * N, torch.float32, sc.SENTINEL, dev, strided=False)   # packed
    k_ptr, v_ptr = kv.view.data_ptr(), kv.view.data_ptr() + C * kv.buf.element_size()
    K.call("cmx_sra_attn_fwd", q.view.data_ptr(), k_ptr, v_ptr, o.view.data_ptr(), lse.view.data_ptr(), Bt, N, Nk,
           heads, D, C + 8, 2 * C + 8, C + 8, scale, code, K.stream())
    torch.cuda.synchronize()
    # the backward reads o and lse as inputs: NaN around them
    o_in = Guarded((Bt, N, C), C + 8, dtype, nan, dev, o.packed().cpu())
    lse_in = Guarded((1, 1, Bt * heads * N), Bt * heads * N, torch.float32, nan, dev, lse.packed().cpu(), strided=False)
    ws = K._ws(K.query("cmx_sra_attn_bwd_workspace", Bt, N, Nk, heads, D), dev)
    K.call("cmx_sra_attn_bwd", q.view.data_ptr(), k_ptr, v_ptr, o_in.view.data_ptr(), do.view.data_ptr(),
           lse_in.view.data_ptr(), dq.view.data_ptr(), dkv.view.data_ptr(),
           dkv.view.data_ptr() + C * dkv.buf.element_size(), K.ptr(ws), Bt, N, Nk, heads, D, C + 8, 2 * C + 8, C + 8,
           C + 8, C + 8, 2 * C + 8, scale, code, K.stream())
    torch.cuda.synchronize()
    for name, g in dict(q=q, kv=kv, do=do, o_in=o_in, lse_in=lse_in).items():
        assert g.unchanged(), f"{case.name}: input {name} was written"
    for name, g in dict(o=o, lse=lse, dq=dq, dkv=dkv).items():
        assert g.outside_unchanged(), f"{case.name}: a store outside the logical {name}"
    return sc.Result(o.packed(), lse.packed().view(Bt, heads, N), dq.packed(), dkv.packed())


CONTAIN_RUNS = [(c, dt) for c in sc.CONTAINMENT for dt in c.dtypes]


@pytest.mark.parametrize("run", CONTAIN_RUNS, ids=[sc.run_id((c, dt, "contain")) for c, dt in CONTAIN_RUNS])
def test_sra_containment(dev, run):
    """strided, guarded tensors: no store outside the logical tensors (a ragged 64-row tile's rows past
    N, the stride gaps), no read of the NaN around the inputs reaches a result (0 x NaN in an MFMA), and
    the results are bit-equal to the packed run"""
    from rgbx_semantic_segmentation_amd import kernels as K
    case, dtype = run
    x = sc.make_inputs(case, "random", dtype)
    with knobs(**case.knobs):
        for seq in ((1, 0) if case.both_dq else (1,)):
            K.tune("SRA_DQ_SEQ", seq)
            assert_plan(K, case, dtype, **(dict(dq_seq=bool(seq)) if case.both_dq else {}))
            # the guarded pointers are 16-B aligned with strides % 8 == 0: the same plan
            packed = run_packed(K, case, x, dtype, dev)
            guarded = run_guarded(K, case, x, dtype, dev)
            for name, a, b in zip(sc.Result._fields, guarded, packed):
                assert torch.isfinite(a).all(), (case.name, name, seq)
                assert torch.equal(bits(a), bits(b)), (case.name, name, seq)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("what", ["stride", "head_dim"])
def test_sra_refusals(dev, dtype, what):
    """a row stride that is no multiple of 8 elements, and D = 48, are refused by forward and backward
    before anything is launched: the outputs keep their sentinel"""
    from rgbx_semantic_segmentation_amd import kernels as K
    from rgbx_semantic_segmentation_amd._lib import CMXError
    Bt, N, Nk, heads = 2, 70, 40, 2
    D = 48 if what == "head_dim" else 64
    C = heads * D
    ld = C + 4 if what == "stride" else C
    code = K.dtype_code(torch.empty(0, dtype=dtype))
    q = torch.ones(Bt * N * ld + 64, device=dev, dtype=dtype)
    kv = torch.ones(Bt, Nk, 2 * C, device=dev, dtype=dtype)
    outs = [torch.full((Bt * N * ld + 64,), sc.SENTINEL, device=dev, dtype=dtype) for _ in range(2)]
    dkv = torch.full((Bt, Nk, 2 * C), sc.SENTINEL, device=dev, dtype=dtype)
    lse = torch.full((Bt, heads, N), sc.SENTINEL, device=dev)
    ws = K._ws(K.query("cmx_sra_attn_bwd_workspace", Bt, N, Nk, heads, 64), dev)
    k_ptr, v_ptr = kv.data_ptr(), kv.data_ptr() + C * kv.element_size()
    with knobs():
        with pytest.raises(CMXError):
            K.call("cmx_sra_attn_fwd", q.data_ptr(), k_ptr, v_ptr, outs[0].data_ptr(), lse.data_ptr(), Bt, N, Nk,
                   heads, D, ld, 2 * C, ld, 0.125, code, K.stream())
        with pytest.raises(CMXError):
            K.call("cmx_sra_attn_bwd", q.data_ptr(), k_ptr, v_ptr, q.data_ptr(), q.data_ptr(), lse.data_ptr(),
                   outs[1].data_ptr(), dkv.data_ptr(), dkv.data_ptr() + C * dkv.element_size(), K.ptr(ws), Bt, N,
                   Nk, heads, D, C if what == "stride" else ld, 2 * C, C if what == "stride" else ld,
                   C if what == "stride" else ld, ld, 2 * C, 0.125, code, K.stream())
    torch.cuda.synchronize()
    for t in outs + [dkv, lse]:
        assert (t == sc.SENTINEL).all()
