"""ProbOhemCrossEntropy2d on the fused upsample + loss path on the GPU (cmx_upsample_ohem_fwd_adj,
cmx_ohem_select / functions.UpsampleOhemF) against the fp64 restatement of tests/ohem_cases.py: the
target probabilities, the exact select on crafted keys, the fused path's selection on its own py, loss
and gradient at the bounds of tests/loss_cases.py, and the structural cases (nothing dropped, dropped
pixels, all ignored, containment, determinism, shape envelope, graph replay, the model, train.py)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import ohem_cases as oc  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = torch.float32
INF = float("inf")
ids = lambda v: str(v).replace("torch.", "")  # noqa: E731


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def fused(dev, shape, dtype, lg, lab, thresh, min_kept):
    """The entry point itself: (out (4), counts (3), py (B, H, W), adj (B, h, w, K)), each filled with
    NaN / -7 before the call."""
    from rgbx_semantic_segmentation_amd import kernels as Kn
    B, h, w, K = shape
    x, labd = lg.to(dev, dtype).contiguous(), lab.to(dev)
    nan = float("nan")
    out, py = torch.full((4,), nan, device=dev), torch.full((B, 4 * h, 4 * w), nan, device=dev)
    adj = torch.full((B, h, w, K), nan, device=dev)
    counts = torch.full((3,), -7, dtype=torch.int64, device=dev)
    ws = Kn._ws(Kn.query("cmx_upsample_ohem_workspace", B, h, w), dev)
    Kn.call("cmx_upsample_ohem_fwd_adj", x, labd, adj, out, py, counts, ws, B, h, w, 4 * h, 4 * w, K, oc.IGNORE,
            float(thresh), int(min_kept), Kn.dtype_code(x))
    torch.cuda.synchronize()
    return out, counts, py, adj


def run(dev, shape, dtype, lg, lab, thresh, min_kept):
    """The product path: builder's plan of the criterion object -> UpsampleOhemF.  Returns (loss,
    dlogits, out, counts) with dloss = 0.7."""
    from rgbx_semantic_segmentation_amd.functions import UpsampleOhemF
    from rgbx_semantic_segmentation_amd.models.builder import OhemSpec, _loss_plan
    from rgbx_semantic_segmentation_amd.utils.loss_opr import ProbOhemCrossEntropy2d
    B, h, w, K = shape
    ignore, spec, weight = _loss_plan(ProbOhemCrossEntropy2d(oc.IGNORE, thresh=thresh, min_kept=min_kept))
    assert isinstance(spec, OhemSpec) and ignore == oc.IGNORE and weight is None
    x = lg.to(dev, dtype).requires_grad_(True)
    loss = UpsampleOhemF.apply(x, lab.to(dev), (B, h, w, 4 * h, 4 * w, K), ignore, spec)
    out, counts = UpsampleOhemF.last
    (loss * oc.DLOSS).backward()
    torch.cuda.synchronize()
    return loss.detach(), x.grad, out, counts


def plain_ce(dev, shape, dtype, lg, lab):
    from rgbx_semantic_segmentation_amd.functions import UpsampleCEF
    B, h, w, K = shape
    x = lg.to(dev, dtype).requires_grad_(True)
    loss = UpsampleCEF.apply(x, lab.to(dev), (B, h, w, 4 * h, 4 * w, K), oc.IGNORE)
    (loss * oc.DLOSS).backward()
    torch.cuda.synchronize()
    return loss.detach(), x.grad


# ------------------------------------------------------------------------ 1. target probabilities
@pytest.mark.parametrize("dtype", oc.DTYPES, ids=ids)
@pytest.mark.parametrize("name", oc.SMALL)
def test_target_probabilities_and_counts(dev, name, dtype):
    """py at valid pixels within 2e-5 absolute of fp64 (the bound MARGIN is 5x of), the sentinel at the
    others, n_valid and n_below exact."""
    c = oc.CASES[name]
    lg, lab = oc.make_inputs(c.shape)
    out, counts, py, _ = fused(dev, c.shape, dtype, lg, lab, c.thresh, c.min_kept)
    want, valid = oc.target_prob(c.shape, dtype)
    got = py.double().cpu()
    err = (got - want)[valid].abs().max().item()
    print(f"ohem py {name} {dtype}: max abs err {err:.3e}")
    assert err <= oc.PY_TOL
    assert torch.equal(got[~valid], torch.full_like(got[~valid], oc.SENTINEL))
    assert counts[0].item() == c.n_valid and counts[1].item() == c.n_below


# ------------------------------------------------------------------------ 2. the select is exact
def _chain(start, n):
    v = torch.empty(n, dtype=F32)
    v[0] = start
    return (v[:1].view(torch.int32) + torch.arange(n, dtype=torch.int32)).view(F32)   # nextafter chain upward


def _select_cases():
    g = torch.Generator().manual_seed(11)
    u = lambda n: torch.rand(n, generator=g)  # noqa: E731
    shuffle = lambda v: v[torch.randperm(v.numel(), generator=g)]  # noqa: E731
    same = torch.full((5000,), 0.3)
    ties = shuffle(torch.cat([torch.full((1000,), 0.1), torch.full((3000,), 0.2), torch.full((1000,), 0.9)]))
    chain = shuffle(_chain(0.7, 4096))
    tiny = torch.tensor([0.0, 1e-45, 3e-42, 1e-39, 1.1754944e-38, 1.0, 1.0, 0.0, 0.5, 1e-40], dtype=F32).repeat(40)
    special = torch.stack([tiny, torch.full_like(tiny, oc.SENTINEL)], 1).flatten()     # sentinels interleaved
    odd = torch.cat([u(300), torch.tensor([float("nan"), -1.0, -0.0, INF, 3.0, 2.0, -INF])])
    cases = {"equal_k1": (same, 0.1, 1), "equal_kmid": (same, 0.1, 2500), "equal_kn": (same, 0.1, 5000),
             "ties_straddle": (ties, 0.05, 2000), "chain_low_mantissa": (chain, 0.5, 1234),
             "special_k1": (special, -1.0, 1), "special_zeros": (special, -1.0, 80), "special_denorm": (special, -1.0, 130),
             "special_one": (special, 0.75, 399), "special_thresh0": (special, 0.0, 50),
             "other_bit_patterns": (odd, 0.01, 150)}
    for n in (1, 257, 100003):
        v = u(n)
        cases[f"n{n}_k1"] = (v, -1.0, 1)
        cases[f"n{n}_kmid"] = (v, 0.0, (n + 1) // 2)
        cases[f"n{n}_kn"] = (v, 0.2, n)                  # k = n_valid: threshold = the largest key
        cases[f"n{n}_kn1"] = (v, 0.2, n + 1)             # k = n_valid + 1: +inf, nothing dropped
    v = u(100003)
    kth = torch.sort(v).values[49999].item()
    cases["thresh_above_kth"] = (v, kth + 1e-3, 50000)
    cases["thresh_below_kth"] = (v, kth - 1e-3, 50000)
    cases["k0"] = (v, 0.5, 0)
    cases["uniform_1e6"] = (u(10 ** 6), 0.3, 400000)
    return cases


SELECT_CASES = _select_cases()


@pytest.mark.parametrize("name", list(SELECT_CASES))
def test_select_is_exact_on_crafted_keys(dev, name):
    """cmx_ohem_select against torch.sort on the CPU: the threshold bit for bit, the counts exactly."""
    from rgbx_semantic_segmentation_amd import kernels as Kn
    keys, thresh, k = SELECT_CASES[name]
    n = keys.numel()
    d = keys.to(dev)
    thr = torch.full((1,), float("nan"), device=dev)
    counts = torch.full((3,), -7, dtype=torch.int64, device=dev)
    ws = Kn._ws(Kn.query("cmx_ohem_select_workspace", n), dev)
    Kn.call("cmx_ohem_select", d, n, float(thresh), int(k), thr, counts, ws)
    torch.cuda.synchronize()
    w_thr, n_valid, n_below, n_kept = oc.host_rule(keys, thresh, k)
    print(f"select {name}: threshold {thr.item()!r} counts {counts.tolist()}")
    assert counts.tolist() == [n_valid, n_below, n_kept]
    assert torch.equal(bits(thr), bits(torch.tensor([w_thr], dtype=F32))), (thr.item(), w_thr)
    assert torch.equal(bits(d), bits(keys))           # the keys are read only
    if name == "ties_straddle":
        assert thr.item() == torch.tensor(0.2).item() and n_kept == 4000


# ------------------------------------------------------------------------ 3. fused path: its own py
@pytest.mark.parametrize("name,dtype", oc.CASE_DTYPES, ids=ids)
def test_fused_path_selects_on_its_own_py(dev, name, dtype):
    """The host rule applied to the returned py in fp32 gives out[3] bitwise and the counts exactly;
    out[2] (the gradient pass's own kept count) agrees."""
    c = oc.CASES[name]
    lg, lab = oc.make_inputs(c.shape)
    out, counts, py, adj = fused(dev, c.shape, dtype, lg, lab, c.thresh, c.min_kept)
    w_thr, n_valid, n_below, n_kept = oc.host_rule(py.cpu().flatten(), c.thresh, c.min_kept)
    assert counts.tolist() == [n_valid, n_below, n_kept]
    assert torch.equal(bits(out[3:]), bits(torch.tensor([w_thr], dtype=F32))), (out[3].item(), w_thr)
    assert out[2].item() == n_kept and out[1].item() == torch.tensor(1.0 / n_kept, dtype=F32).item()
    assert torch.isfinite(adj).all()


# ------------------------------------------------------------------------ 4. loss and gradient
@pytest.mark.parametrize("name,dtype", oc.CASE_DTYPES, ids=ids)
def test_loss_and_gradient_against_fp64(dev, name, dtype):
    c = oc.CASES[name]
    lg, lab = oc.make_inputs(c.shape)
    loss, dl, out, counts = run(dev, c.shape, dtype, lg, lab, c.thresh, c.min_kept)
    e = oc.expected(name, dtype)
    le = abs(loss.item() - e.loss.item()) / abs(e.loss.item())
    ge = oc.lc.relerr(dl.view_as(e.dlogits), e.dlogits)
    te = 0.0 if e.threshold == INF and out[3].item() == INF else abs(out[3].item() - e.threshold)
    print(f"ohem {name} {dtype}: loss rel err {le:.3e}, dlogits rel err {ge:.3e}, threshold abs err {te:.3e}")
    assert counts.tolist() == [c.n_valid, c.n_below, c.n_kept] == [e.n_valid, e.n_below, e.n_kept]
    assert te <= oc.PY_TOL
    assert le < oc.LOSS_TOL[dtype], (le, loss.item(), e.loss.item())
    assert ge < oc.TOL[dtype], ge


# ------------------------------------------------------------------------ 5. nothing dropped
@pytest.mark.parametrize("name", ["s0_nofilter", "s0_minkept0", "s2_all"])
def test_nothing_dropped_is_plain_ce(dev, name):
    c = oc.CASES[name]
    lg, lab = oc.make_inputs(c.shape)
    loss, dl, out, counts = run(dev, c.shape, F32, lg, lab, c.thresh, c.min_kept)
    ce, dce = plain_ce(dev, c.shape, F32, lg, lab)
    same = torch.equal(loss, ce) and torch.equal(dl, dce)
    print(f"ohem {name} vs plain CE: bits {'equal' if same else 'differ'}; loss {loss.item()!r} {ce.item()!r}")
    assert counts[2].item() == counts[0].item() == c.n_valid
    assert abs(loss.item() - ce.item()) <= 1e-6 * abs(ce.item())
    assert oc.lc.relerr(dl, dce) <= 1e-6


# ------------------------------------------------------------------------ 6. dropped pixels
@pytest.mark.parametrize("name", ["s1_thresh_low", "s2_kth"])
def test_dropped_pixels_carry_nothing(dev, name):
    """dlogits sums to zero over the classes at every low-res pixel (the adjoint of a zero-sum
    full-resolution gradient), and plain CE on labels with the dropped pixels set to ignore gives the
    same loss and dlogits."""
    c = oc.CASES[name]
    B, h, w, K = c.shape
    lg, lab = oc.make_inputs(c.shape)
    loss, dl, out, counts = run(dev, c.shape, F32, lg, lab, c.thresh, c.min_kept)
    _, _, py, _ = fused(dev, c.shape, F32, lg, lab, c.thresh, c.min_kept)
    assert counts[2].item() == c.n_kept < c.n_valid
    gmax = dl.abs().max().item()
    assert dl.double().view(B, h, w, K).sum(-1).abs().max().item() <= oc.TOL[F32] * gmax
    kept = (lab != oc.IGNORE) & (py.cpu() <= out[3].item())
    assert int(kept.sum()) == c.n_kept
    ce, dce = plain_ce(dev, c.shape, F32, lg, torch.where(kept, lab, torch.full_like(lab, oc.IGNORE)))
    assert abs(loss.item() - ce.item()) <= 1e-6 * abs(ce.item())
    assert oc.lc.relerr(dl, dce) <= 1e-6


# ------------------------------------------------------------------------ 7. all ignored
def test_all_ignored_and_out_of_range_labels(dev):
    shape = oc.SHAPES[2]
    K = shape[3]
    lg, lab = oc.lc.make_inputs(shape, ignored="all")
    loss, dl, out, counts = run(dev, shape, F32, lg, lab, 0.6, 256)
    assert torch.isnan(loss).item() and torch.count_nonzero(dl).item() == 0
    assert counts.tolist() == [0, 0, 0] and out[3].item() == INF and out[1].item() == 0.0
    # labels outside [0, K) that are not the ignore value count as ignored: the same bits
    lg, lab = oc.make_inputs(shape)
    bad = lab.clone()
    bad[0, 1, 2], bad[1, 40, 33], bad[0, 50, 60] = K + 3, -1, K
    ign = torch.where((bad < 0) | (bad >= K), torch.full_like(bad, oc.IGNORE), bad)
    for thresh, k in ((0.6, 256), (0.091, 4880)):
        a = run(dev, shape, F32, lg, bad, thresh, k)
        b = run(dev, shape, F32, lg, ign, thresh, k)
        for u, v in zip(a, b):
            assert torch.equal(u, v)
        assert torch.isfinite(a[0]).item() and a[3][0].item() == 5422 - 3


# ------------------------------------------------------------------------ 8. containment
def test_containment(dev):
    """adj, py, counts, out and dlogits sit inside larger pattern-filled allocations with guards before
    and after: the kernels write exactly their elements and the guards come back bit-equal."""
    from rgbx_semantic_segmentation_amd import kernels as Kn
    name, dtype = "s2_kth", torch.bfloat16
    c = oc.CASES[name]
    B, h, w, K = c.shape
    lg, lab = oc.make_inputs(c.shape)
    x, labd = lg.to(dev, dtype).contiguous(), lab.to(dev)
    n, npx, guard = B * h * w * K, B * 16 * h * w, 3 * w * K
    nan = float("nan")
    bufs = {"adj": (torch.full((n + 2 * guard,), nan, device=dev), n, torch.int32),
            "py": (torch.full((npx + 2 * guard,), nan, device=dev), npx, torch.int32),
            "out": (torch.full((4 + 2 * guard,), nan, device=dev), 4, torch.int32),
            "counts": (torch.full((3 + 2 * guard,), -7, dtype=torch.int64, device=dev), 3, torch.int64),
            "dl": (torch.full((n + 2 * guard,), nan, device=dev).to(dtype), n, torch.int16)}
    v = {k: b[guard:guard + m] for k, (b, m, _) in bufs.items()}
    before = {k: b.view(it).clone() for k, (b, m, it) in bufs.items()}
    ws = Kn._ws(Kn.query("cmx_upsample_ohem_workspace", B, h, w), dev)
    Kn.call("cmx_upsample_ohem_fwd_adj", x, labd, v["adj"], v["out"], v["py"], v["counts"], ws, B, h, w, 4 * h, 4 * w, K,
            oc.IGNORE, c.thresh, c.min_kept, Kn.dtype_code(x))
    dloss = torch.full((1,), oc.DLOSS, device=dev)
    Kn.call("cmx_upsample_ce_bwd_scale", v["adj"], dloss, v["out"], v["dl"], n, Kn.dtype_code(x))
    torch.cuda.synchronize()
    for k, (b, m, it) in bufs.items():
        now = b.view(it)
        assert torch.equal(now[:guard], before[k][:guard]) and torch.equal(now[guard + m:], before[k][guard + m:]), k
        if k != "counts":
            assert torch.isfinite(v[k]).all(), k
    e = oc.expected(name, dtype)
    assert v["counts"].tolist() == [c.n_valid, c.n_below, c.n_kept]
    assert abs(v["out"][0].item() - e.loss.item()) / e.loss.item() < oc.LOSS_TOL[dtype]
    assert oc.lc.relerr(v["dl"].view(B, h, w, K), e.dlogits) < oc.TOL[dtype]


# ------------------------------------------------------------------------ 9. determinism
@pytest.mark.parametrize("name", ["s2_kth", "big_kth"])
def test_same_call_twice_gives_the_same_bits(dev, name):
    """No floating-point atomics: out, counts, py and adj of two calls are torch.equal."""
    c = oc.CASES[name]
    lg, lab = oc.make_inputs(c.shape)
    a = fused(dev, c.shape, torch.bfloat16, lg, lab, c.thresh, c.min_kept)
    b = fused(dev, c.shape, torch.bfloat16, lg, lab, c.thresh, c.min_kept)
    for u, v in zip(a, b):
        assert torch.isfinite(u).all() and torch.equal(u, v)
    assert a[1][2].item() == c.n_kept


# ------------------------------------------------------------------------ 10. shape envelope
def test_shape_envelope_raises(dev):
    from rgbx_semantic_segmentation_amd.functions import UpsampleOhemF
    x = torch.zeros(1, 2, 2, 9, device=dev)
    lab = torch.zeros(1, 8, 9, dtype=torch.int64, device=dev)
    with pytest.raises(NotImplementedError, match="2x2 -> 8x9"):
        UpsampleOhemF.apply(x, lab, (1, 2, 2, 8, 9, 9), 255, (0.6, 256))
    x = torch.zeros(1, 2, 2, 41, device=dev)
    lab = torch.zeros(1, 8, 8, dtype=torch.int64, device=dev)
    with pytest.raises(NotImplementedError, match="K=41"):
        UpsampleOhemF.apply(x, lab, (1, 2, 2, 8, 8, 41), 255, (0.6, 256))


# ------------------------------------------------------------------------ 11. graph replay
def test_graph_replay_chooses_the_regime_on_the_device(dev):
    """Forward + backward captured once with s1_thresh's parameters; the static logits buffer then takes
    an input of the thresh regime and one of the kth regime.  Each replay equals the eager call bit for
    bit: nothing about the regime was fixed at capture.
    The kth-regime input needs fewer than min_kept = 256 pixels at or below thresh = 0.6, which low-res
    logits cannot give under make_inputs' labels (independent per full-res pixel: the 16 pixels of a cell
    want different classes; +8 on the centre pixel's class leaves n_below at 3506 of 3975 on the fp64
    reference, +40 at 3316).  So the labels here are the centre labels held constant over each low-res
    cell, and the boost on the cell's class is +40: n_below 3835 without it, 130 with it (+8: 1745)."""
    from rgbx_semantic_segmentation_amd.functions import UpsampleOhemF
    from rgbx_semantic_segmentation_amd.utils.loss_opr import ProbOhemCrossEntropy2d
    c = oc.CASES["s1_thresh"]
    B, h, w, K = c.shape
    dims, spec = (B, h, w, 4 * h, 4 * w, K), (c.thresh, c.min_kept)
    lg, lab = oc.make_inputs(c.shape)
    centre = lab[:, 2::4, 2::4]
    lab = centre.repeat_interleave(4, 1).repeat_interleave(4, 2)
    boost = torch.zeros_like(lg)
    boost.scatter_(3, centre.clamp(0, K - 1).unsqueeze(3), 40.0 * (centre != oc.IGNORE).unsqueeze(3).double())
    inputs = [lg.float(), (lg + boost).float()]
    crit = ProbOhemCrossEntropy2d(oc.IGNORE, thresh=c.thresh, min_kept=c.min_kept)
    below = [crit.selection(oc.upsampled(v), lab)[3] for v in inputs]
    assert below[0] >= c.min_kept + 100 and below[1] <= c.min_kept - 100, below   # far from the regime boundary
    labd = lab.to(dev)

    def step(x):
        x.grad = None
        loss = UpsampleOhemF.apply(x, labd, dims, oc.IGNORE, spec)
        (loss * oc.DLOSS).backward()
        return loss, UpsampleOhemF.last

    eager = []
    for v in inputs:
        x = v.to(dev).requires_grad_(True)
        loss, (out, counts) = step(x)
        torch.cuda.synchronize()
        eager.append((loss.detach().clone(), x.grad.clone(), out.clone(), counts.clone()))
    assert eager[0][3][1].item() >= c.min_kept > eager[1][3][1].item()
    assert eager[0][2][3].item() == torch.tensor(c.thresh).item() and c.thresh < eager[1][2][3].item() < INF
    xs = inputs[1].to(dev).requires_grad_(True)       # captured on the OTHER regime's input than first replayed
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step(xs)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        loss, (out, counts) = step(xs)
    grad = xs.grad
    for i in (0, 1, 0, 1, 1, 0):
        with torch.no_grad():
            xs.copy_(inputs[i].to(dev))
        grad.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip((loss.detach(), grad, out, counts), eager[i]):
            assert torch.equal(got, want), (i, got, want)


# ------------------------------------------------------------------------ 12. model level
def _model(dev, criterion, dtype="float32", K=9):
    from rgbx_semantic_segmentation_amd.models.builder import EncoderDecoder
    cfg = dict(backbone="mit_b0", num_classes=K, compute_dtype=dtype, decoder_embed_dim=256)
    return EncoderDecoder(cfg, criterion=criterion).to(dev)


def test_model_takes_the_ohem_path(dev, monkeypatch):
    """mit_b0, 64 x 96, batch 2, fp32: the criterion goes through UpsampleOhemF; its loss is >= the plain
    CE loss of the same forward (kept = the pixels with -log p_y >= -log threshold, so their mean cannot be
    smaller); every parameter gradient is finite."""
    from rgbx_semantic_segmentation_amd import functions as Fm
    from rgbx_semantic_segmentation_amd.models.builder import OhemSpec
    from rgbx_semantic_segmentation_amd.utils.loss_opr import ProbOhemCrossEntropy2d
    calls = []
    real = Fm.UpsampleOhemF.apply
    monkeypatch.setattr(Fm.UpsampleOhemF, "apply", lambda *a: (calls.append(a[4]), real(*a))[1])
    torch.manual_seed(0)
    m = _model(dev, ProbOhemCrossEntropy2d(255, thresh=0.05, min_kept=512))
    assert isinstance(m._loss_spec, OhemSpec) and m._loss_spec == (0.05, 512)
    ce = _model(dev, None)
    ce.load_state_dict(m.state_dict(), strict=True)
    m.eval(), ce.eval()
    g = torch.Generator().manual_seed(3)
    rgb, x = torch.randn(2, 3, 64, 96, generator=g).to(dev), torch.randn(2, 3, 64, 96, generator=g).to(dev)
    lab = torch.randint(0, 9, (2, 64, 96), generator=g)
    lab[:, 5:20, 7:30] = 255
    lab = lab.to(dev)
    loss = m(rgb, x, lab)
    loss.backward()
    loss_ce = ce(rgb, x, lab)
    torch.cuda.synchronize()
    out, counts = Fm.UpsampleOhemF.last
    print(f"ohem model: loss {loss.item():.6f} plain CE {loss_ce.item():.6f} counts {counts.tolist()}")
    assert calls == [m._loss_spec] and type(loss.grad_fn).__name__ == "UpsampleOhemFBackward"
    assert 512 <= counts[2].item() < counts[0].item() == int((lab != 255).sum())
    assert torch.isfinite(loss).item() and loss.item() >= loss_ce.item()
    assert torch.isfinite(m.store.grad).all() and m.store.grad.abs().max() > 0
    for n, p in m.named_parameters():
        assert p.grad is None or torch.isfinite(p.grad).all(), n


def test_train_loop_ohem_and_amp(dev, monkeypatch):
    """train.py --criterion ProbOhemCrossEntropy2d --ohem-min-kept 512: 3 iterations give a finite loss;
    once under --use-mixed-precision (the GradScaler path)."""
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    import train
    base = ["--backbone", "mit_b0", "--num-classes", "9", "--height", "64", "--width", "96", "--batch-size", "2",
            "--niters-per-epoch", "3", "--nepochs", "1", "--warm-up-epoch", "0", "--lr", "1e-4",
            "--criterion", "ProbOhemCrossEntropy2d", "--ohem-min-kept", "512"]
    l1 = train.main(base + ["--compute-dtype", "float32"])
    assert l1 == l1 and 0 < l1 < INF
    l2 = train.main(base + ["--use-mixed-precision"])
    assert l2 == l2 and 0 < l2 < INF
