"""Fused SGD with momentum (csrc/sgdm.hip, optim.FusedSGD, ``train.py --optimizer SGDM``) against
``torch.optim.SGD(..., foreach=False)`` on the CPU in fp64.

The bound for a tensor is ``2 E_ref + u max|ref|``: E_ref is the worst absolute error of the same
torch.optim.SGD run in fp32 on the CPU against the fp64 run (computed here, deterministic) and
u = 2^-23, the project's "2 E + one ulp" with torch's own fp32 optimizer as the yardstick.  Bit
equality with torch is not asked (either side may or may not fuse its multiply-adds).  A skipped or
no-op step must fail: in the flat-buffer cases the median |dp| of every step over the non-frozen
elements (from the fp64 reference) is at least 100 x the bound.
"""
import copy
import functools
import gc

import pytest
import torch

from oracle.cmx_ref import EncoderDecoder as RefModel, CMXConfig, DropPath
from oracle.train_ref import WarmUpPolyLR, group_weight, train_steps

pytestmark = pytest.mark.gpu

U = 2.0 ** -23
LRS = (1e-2, 5e-3, 2e-2, 1e-2)
MOMENTUM, WD = 0.9, 0.01
GUARD = 64
# NaN bit patterns of the guards (a stray write, or a read that reaches the arithmetic, shows)
NAN32 = 0x7FC0DEAD
NAN16 = {torch.bfloat16: 0x7FC1, torch.float16: 0x7E01}
SHADOW_INIT = 0x1234            # what the shadow holds before the first step (must be overwritten)
BUF_FROZEN = 7.0                # what the frozen blocks of buf hold (must stay)

VARIANTS = {"momentum": (MOMENTUM, False), "nesterov": (MOMENTUM, True), "plain": (0.0, False)}
SIZES = {"n64": (64, 0), "n1088": (1088, 0), "n64000_cap3": (64000, 3), "n64000": (64000, 0)}
SHADOWS = {"noshadow": None, "bf16": torch.bfloat16, "fp16": torch.float16}


# ------------------------------------------------------------------ flat-buffer inputs and reference
def _flags(n):
    return torch.tensor([(1, 0, 2)[b % 3] for b in range(n // 64)], dtype=torch.uint8)


@functools.lru_cache(maxsize=None)
def _inputs(n):
    """p ~ 0.05 N(0,1), four g ~ 0.02 N(0,1) (NaN in the frozen blocks), per-element flags."""
    gen = torch.Generator().manual_seed(1234 + n)
    p = 0.05 * torch.randn(n, generator=gen)
    gs = [0.02 * torch.randn(n, generator=gen) for _ in LRS]
    fe = _flags(n).repeat_interleave(64)
    for g in gs:
        g[fe == 2] = float("nan")
    return p, gs, fe


def _torch_sgd(p, gs, fe, momentum, nesterov, dtype, gmul=1.0):
    """torch.optim.SGD over the flag-1 and flag-0 elements as two groups (the frozen ones are in
    no group); [(p, buf)] after every step, scattered back to flat order."""
    sel = [fe == 1, fe == 0]
    params = [torch.nn.Parameter(p[m].to(dtype).clone()) for m in sel]
    groups = [dict(params=[params[0]]), dict(params=[params[1]], weight_decay=0.0)]
    groups = [g for g, q in zip(groups, params) if q.numel()]
    opt = torch.optim.SGD(groups, lr=LRS[0], momentum=momentum, weight_decay=WD, nesterov=nesterov, foreach=False)
    out = []
    for lr, g in zip(LRS, gs):
        for grp in opt.param_groups:
            grp["lr"] = lr
        for q, m in zip(params, sel):
            q.grad = (g[m] * gmul).to(dtype)
        opt.step()
        pf, bf = p.to(dtype).clone(), torch.zeros(p.numel(), dtype=dtype)
        for q, m in zip(params, sel):
            pf[m] = q.detach()
            if momentum != 0 and q.numel():
                bf[m] = opt.state[q]["momentum_buffer"]
        out.append((pf, bf))
    return out


@functools.lru_cache(maxsize=None)
def _reference(n, variant):
    """Per step: fp64 (p, buf), the bounds of p and buf, and the median |dp| over non-frozen elements."""
    momentum, nesterov = VARIANTS[variant]
    p, gs, fe = _inputs(n)
    r64 = _torch_sgd(p, gs, fe, momentum, nesterov, torch.float64)
    r32 = _torch_sgd(p, gs, fe, momentum, nesterov, torch.float32)
    live = fe != 2
    steps, prev = [], p.double()
    for (p64, b64), (p32, b32) in zip(r64, r32):
        bound_p = 2 * (p32.double() - p64)[live].abs().max().item() + U * p64[live].abs().max().item()
        bound_b = 2 * (b32.double() - b64)[live].abs().max().item() + U * b64[live].abs().max().item()
        moved = (p64 - prev)[live].abs().median().item()
        steps.append((p64, b64, bound_p, bound_b, moved))
        prev = p64
    return steps


# ------------------------------------------------------------------ guarded device buffers
class _Guarded:
    """A device buffer of n elements with GUARD elements of a NaN bit pattern on both sides."""

    def __init__(self, n, dtype, dev, fill=None):
        self.n, self.dtype = n, dtype
        self.idt, self.pattern = (torch.int32, NAN32) if dtype == torch.float32 else (torch.int16, NAN16[dtype])
        self.raw = torch.full((n + 2 * GUARD,), self.pattern, dtype=self.idt, device=dev)
        self.t = self.raw.view(dtype)[GUARD:GUARD + n]
        if fill is not None:
            self.t.copy_(fill)

    def bits(self):
        return self.raw[GUARD:GUARD + self.n].cpu()

    def guards_intact(self):
        r = self.raw.cpu()
        return bool((r[:GUARD] == self.pattern).all() and (r[GUARD + self.n:] == self.pattern).all())


class _Flat:
    def __init__(self, n, dev, momentum, shadow_dtype, p, fe):
        self.n, self.momentum = n, momentum
        self.p = _Guarded(n, torch.float32, dev, p)
        self.g = _Guarded(n, torch.float32, dev)
        self.buf = None
        if momentum != 0:
            self.buf = _Guarded(n, torch.float32, dev, torch.where(fe == 2, BUF_FROZEN, 0.0))
        self.shadow = None
        if shadow_dtype is not None:
            self.shadow = _Guarded(n, shadow_dtype, dev)
            self.shadow.raw[GUARD:GUARD + n] = SHADOW_INIT
        self.code = {None: 0, torch.bfloat16: 1, torch.float16: 2}[shadow_dtype]
        self.flags = _flags(n).to(dev)
        self.lr = torch.zeros(1, dtype=torch.float32, device=dev)

    def all(self):
        return [b for b in (self.p, self.g, self.buf, self.shadow) if b is not None]

    def step(self, g, lr, nesterov=False, grad_scale=1.0, loss_scale=None, found_inf=None, max_blocks=0):
        from rgbx_semantic_segmentation_amd._lib import call, ptr, stream
        self.g.t.copy_(g)
        self.lr.fill_(lr)
        call("cmx_sgdm_step", ptr(self.p.t), ptr(self.g.t), ptr(self.buf.t if self.buf else None),
             ptr(self.shadow.t if self.shadow else None), self.code, ptr(self.flags), self.n, ptr(self.lr),
             self.momentum, WD, int(nesterov), grad_scale, ptr(loss_scale), ptr(found_inf), max_blocks, stream())
        torch.cuda.synchronize()


# ------------------------------------------------------------------ 1. flat buffers through the C-ABI
@pytest.mark.parametrize("shadow", list(SHADOWS))
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("size", list(SIZES))
def test_flat_sgdm_step_matches_torch_sgd(dev, size, variant, shadow):
    n, max_blocks = SIZES[size]
    momentum, nesterov = VARIANTS[variant]
    sdt = SHADOWS[shadow]
    p0, gs, fe = _inputs(n)
    ref = _reference(n, variant)
    live, frozen = fe != 2, fe == 2
    f = _Flat(n, dev, momentum, sdt, p0, fe)
    p0_bits = f.p.bits()
    for it, (lr, g) in enumerate(zip(LRS, gs)):
        f.step(g, lr, nesterov=nesterov, max_blocks=max_blocks)
        p64, b64, bound_p, bound_b, moved = ref[it]
        p = f.p.t.cpu()
        ep = (p.double() - p64)[live].abs().max().item()
        eb = 0.0
        if f.buf is not None:
            b = f.buf.t.cpu()
            eb = (b.double() - b64)[live].abs().max().item()
        print(f"{size} {variant} {shadow} step {it}: |p - ref| {ep:.2e} (bound {bound_p:.2e}), |buf - ref| {eb:.2e} "
              f"(bound {bound_b:.2e}), median |dp| {moved:.2e} = {moved / bound_p:.0f} x bound")
        assert moved >= 100 * bound_p, (it, moved, bound_p)          # the moved condition
        assert ep <= bound_p, (it, ep, bound_p)
        if f.buf is not None:
            assert eb <= bound_b, (it, eb, bound_b)
            assert bool((b[frozen] == BUF_FROZEN).all()), it
        assert torch.equal(f.p.bits()[frozen], p0_bits[frozen]), it
        if f.shadow is not None:
            sh = f.shadow.t.cpu()
            assert torch.equal(sh[live], p.to(sdt)[live]), it
            assert bool((f.shadow.bits()[frozen] == SHADOW_INIT).all()), it
        for buf in f.all():
            assert buf.guards_intact(), it


# ------------------------------------------------------------------ 2. scales
def _run_scaled(dev, gmul, steps=2, **kw):
    n = 1088
    p0, gs, fe = _inputs(n)
    f = _Flat(n, dev, MOMENTUM, torch.bfloat16, p0, fe)
    for lr, g in list(zip(LRS, gs))[:steps]:
        f.step(g * gmul, lr, **kw)
    return f


def _same_bits(a, b):
    return all(torch.equal(x.raw.cpu(), y.raw.cpu()) for x, y in ((a.p, b.p), (a.buf, b.buf), (a.shadow, b.shadow)))


def test_grad_scale_is_exact_for_a_power_of_two(dev):
    base = _run_scaled(dev, 0.125, grad_scale=1.0)
    p0, _, fe = _inputs(1088)
    assert (base.p.t.cpu() != p0)[fe != 2].float().mean().item() > 0.99      # the non-frozen elements moved
    assert _same_bits(_run_scaled(dev, 1.0, grad_scale=0.125), base)


def test_loss_scale_is_exact_for_a_power_of_two(dev):
    scale = torch.full((1,), 1024.0, device=dev)
    clear = torch.zeros(1, device=dev)
    base = _run_scaled(dev, 1.0)
    assert _same_bits(_run_scaled(dev, 1024.0, loss_scale=scale), base)
    assert _same_bits(_run_scaled(dev, 1024.0, loss_scale=scale, found_inf=clear), base)


def test_found_inf_skips_the_whole_step(dev):
    n = 1088
    p0, gs, fe = _inputs(n)
    f = _Flat(n, dev, MOMENTUM, torch.bfloat16, p0, fe)
    f.step(gs[0], LRS[0])                                  # a state that is not all zeros
    before = [b.raw.cpu().clone() for b in (f.p, f.buf, f.shadow)]
    found = torch.ones(1, device=dev)
    f.step(gs[1], LRS[1], loss_scale=torch.ones(1, device=dev), found_inf=found)
    for b, was in zip((f.p, f.buf, f.shadow), before):
        assert torch.equal(b.raw.cpu(), was)               # interior and guards, bit for bit
    assert f.g.guards_intact() and found.item() == 1.0


# ------------------------------------------------------------------ model-level helpers
BACKBONE, K, B, H, W = "mit_b0", 9, 2, 128, 160
LR = 1e-2


def _pair(dev, dtype="float32", seed=0):
    from rgbx_semantic_segmentation_amd.models.builder import EncoderDecoder
    torch.manual_seed(seed)
    ref = RefModel(CMXConfig(backbone=BACKBONE, num_classes=K))
    model = EncoderDecoder(dict(backbone=BACKBONE, num_classes=K, compute_dtype=dtype, decoder_embed_dim=512)).to(dev)
    model.load_state_dict(ref.state_dict(), strict=True)
    return ref, model


def _batch(seed=3):
    from rgbx_semantic_segmentation_amd.data import make_batch
    return make_batch(B, H, W, K, seed=seed)


def _torch_opt(ref):
    return torch.optim.SGD(group_weight(ref, LR), lr=LR, momentum=MOMENTUM, weight_decay=WD, foreach=False)


def _fused(model, **kw):
    from rgbx_semantic_segmentation_amd.optim import FusedSGD
    return FusedSGD(model, lr=LR, momentum=MOMENTUM, weight_decay=WD, **kw)


def _buffers(opt_t, ref):
    """{name: momentum_buffer} of a torch.optim.SGD over ``ref``'s parameters."""
    names = {id(p): n for n, p in ref.named_parameters()}
    return {names[id(p)]: opt_t.state[p]["momentum_buffer"] for grp in opt_t.param_groups for p in grp["params"]}


def _gpu_buffers(opt, model):
    sd = opt.state_dict()
    names = {id(p): n for n, p in model.named_parameters()}
    return {names[id(p)]: sd["state"][i]["momentum_buffer"].cpu() for i, p in enumerate(opt._order)}


# ------------------------------------------------------------------ 3. FusedSGD on shared gradients
def test_fused_sgd_matches_torch_sgd_on_shared_gradients(dev):
    ref32, model = _pair(dev)
    ref64 = copy.deepcopy(ref32).double()
    model.eval()
    opt64, opt32, opt = _torch_opt(ref64), _torch_opt(ref32), _fused(model)
    assert [set(g) for g in opt.param_groups] == [set(g) for g in opt32.param_groups]
    assert [len(g["params"]) for g in opt.param_groups] == [len(g["params"]) for g in opt32.param_groups]
    pol = WarmUpPolyLR(LR, 0.9, 100, 2)
    rgb, x, lab = _batch()
    gp = dict(model.named_parameters())
    p32, p64 = dict(ref32.named_parameters()), dict(ref64.named_parameters())
    lr = LR
    for it in range(4):
        model(rgb.to(dev), x.to(dev), lab.to(dev)).backward()
        torch.cuda.synchronize()
        before = model.store.flat.clone()
        for n in p32:                                      # the SAME gradients on all three sides
            p32[n].grad = gp[n].grad.detach().cpu().clone()
            p64[n].grad = p32[n].grad.double()
        opt64.step()
        opt32.step()
        opt.step()
        torch.cuda.synchronize()
        travelled = (model.store.flat - before).norm().item()
        b64, b32, bg = _buffers(opt64, ref64), _buffers(opt32, ref32), _gpu_buffers(opt, model)
        assert set(bg) == set(b64)
        worst_p = worst_b = 0.0
        for n in p64:
            r = p64[n].detach()
            bound = 2 * (p32[n].detach().double() - r).abs().max().item() + U * r.abs().max().item()
            e = (gp[n].detach().cpu().double() - r).abs().max().item()
            worst_p = max(worst_p, e / bound if bound > 0 else float(e > 0))
            assert e <= bound, (it, n, e, bound)
            if n in b64:
                bound = 2 * (b32[n].double() - b64[n]).abs().max().item() + U * b64[n].abs().max().item()
                e = (bg[n].double() - b64[n]).abs().max().item()
                worst_b = max(worst_b, e / bound if bound > 0 else float(e > 0))
                assert e <= bound, (it, n, e, bound)
        print(f"step {it}: lr {lr:.3e}; worst |p - ref| / bound {worst_p:.2f}; worst |buf - ref| / bound {worst_b:.2f}; "
              f"travelled {travelled:.3e}")
        if lr != 0:
            assert travelled > 0, it
        lr = pol.get_lr(it)                                # the LR lands one step late
        for o in (opt64, opt32, opt):
            for grp in o.param_groups:
                grp["lr"] = lr


# ------------------------------------------------------------------ 4. trajectory against the fp64 oracle
def _inject(model, refs, n_calls, seed=7):
    g = torch.Generator().manual_seed(seed)
    bb = model.backbone
    flags = torch.ones(sum(bb.depths), 2, 2 * B)
    bi, per = 0, []
    for s in range(4):
        for i in range(bb.depths[s]):
            for stream, pre in enumerate(("", "extra_")):
                rblk = getattr(refs[0].backbone, f"{pre}block{s + 1}")[i]
                if isinstance(rblk.drop_path, DropPath):
                    mk = [(torch.rand(B, generator=g) > 0.3).double() for _ in range(2)]
                    per.append((f"{pre}block{s + 1}", i, mk))
                    for br in range(2):
                        flags[bi, br, stream * B:(stream + 1) * B] = mk[br].float()
            bi += 1
    d2 = (torch.rand(B, 512, generator=g) > 0.1).double()
    for r in refs:
        for name, i, mk in per:
            getattr(r.backbone, name)[i].drop_path.masks = [m.clone() for _ in range(n_calls) for m in mk]
        r.decode_head.dropout.mask = d2
    model.forced_masks = {"droppath": flags, "dropout2d": d2.float()}


def test_sgd_train_loop_trajectory_vs_oracle(dev):
    """train.py's loop body on both sides for 4 steps, each side computing its own gradients (HIP
    fp32 vs oracle fp64, train mode, injected masks); the thresholds of the AdamW trajectory test."""
    ref, model = _pair(dev)
    ref = ref.double()
    p0 = {n: p.detach().clone() for n, p in ref.named_parameters()}
    opt_t, opt = _torch_opt(ref), _fused(model)
    pol = WarmUpPolyLR(LR, 0.9, 100, 2)
    ref.train()
    model.train()
    steps = 4
    _inject(model, [ref], n_calls=steps)
    batches = [_batch(seed=3 + i) for i in range(steps)]
    gp = dict(model.named_parameters())
    for it, (rgb, x, lab) in enumerate(batches):
        l_ref = train_steps(ref, opt_t, pol, [(rgb.double(), x.double(), lab)], start_iter=it)[0]
        loss = model(rgb.to(dev), x.to(dev), lab.to(dev))
        l_gpu = loss.item()
        opt.zero_grad()
        loss.backward()
        opt.step()
        for grp in opt.param_groups:
            grp["lr"] = pol.get_lr(it)
        torch.cuda.synchronize()
        num = den = 0.0
        for n, p in ref.named_parameters():
            num += (gp[n].detach().cpu().double() - p.detach()).pow(2).sum().item()
            den += (p.detach() - p0[n]).pow(2).sum().item()
        rel = (num / max(den, 1e-300)) ** 0.5
        bt, bg = _buffers(opt_t, ref), _gpu_buffers(opt, model)
        mnum = mden = 0.0
        for n in bt:
            mnum += (bg[n].double() - bt[n]).pow(2).sum().item()
            mden += bt[n].pow(2).sum().item()
        mrel = (mnum / max(mden, 1e-300)) ** 0.5
        print(f"step {it}: loss gpu {l_gpu:.6f} oracle {l_ref:.6f}; |p - p_ref| / |p_ref - p0| {rel:.2e}; "
              f"momentum_buffer rel {mrel:.2e}")
        assert abs(l_gpu - l_ref) / abs(l_ref) < 1e-4, (it, l_gpu, l_ref)
        if den > 0:
            assert rel < 1e-2, (it, rel)
        assert mrel < 1e-3, (it, mrel)


# ------------------------------------------------------------------ 5. checkpoints both ways
def test_restore_reference_sgd_checkpoint_then_step(dev, tmp_path, monkeypatch):
    from rgbx_semantic_segmentation_amd.engine.engine import Engine
    from rgbx_semantic_segmentation_amd.models.builder import EncoderDecoder
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    torch.manual_seed(5)
    ref = RefModel(CMXConfig(backbone=BACKBONE, num_classes=K))
    ref.eval()
    opt_t = _torch_opt(ref)
    pol = WarmUpPolyLR(LR, 0.9, 100, 0)
    rgb, x, lab = _batch(seed=9)
    for it in range(2):
        loss = ref(rgb, x, lab)
        opt_t.zero_grad()
        loss.backward()
        opt_t.step()
        for grp in opt_t.param_groups:
            grp["lr"] = pol.get_lr(it)
    path = tmp_path / "epoch-3.pth"
    torch.save({"model": ref.state_dict(), "optimizer": opt_t.state_dict(), "epoch": 3, "iteration": 5}, path)

    torch.manual_seed(123)                     # different init: everything must come from the file
    model = EncoderDecoder(dict(backbone=BACKBONE, num_classes=K, compute_dtype="float32",
                                decoder_embed_dim=512)).to(dev)
    model.eval()
    opt = _fused(model)
    with Engine(argv=["-c", str(path)]) as e:
        e.register_state(model=model, optimizer=opt)
        e.restore_checkpoint()
        assert e.state.epoch == 4 and e.state.iteration == 5
    gp = dict(model.named_parameters())
    for n, p in ref.named_parameters():
        assert torch.equal(gp[n].detach().cpu(), p.detach()), n
    bt, bg = _buffers(opt_t, ref), _gpu_buffers(opt, model)
    assert set(bt) == set(bg)
    for n in bt:
        assert torch.equal(bg[n], bt[n]), n
    assert opt.param_groups[0]["lr"] == opt.param_groups[1]["lr"] == opt_t.param_groups[0]["lr"]
    assert opt.lr_t.item() == torch.tensor(opt_t.param_groups[0]["lr"], dtype=torch.float32).item()
    # one more step on each side, same batch: the restored state drives the same update
    rgb, x, lab = _batch(seed=10)
    gref = copy.deepcopy(ref).double()
    opt_64 = _torch_opt(gref)
    opt_64.load_state_dict(opt_t.state_dict())        # same group_weight order: state maps by position
    gref(rgb.double(), x.double(), lab).backward()
    opt_64.step()
    model(rgb.to(dev), x.to(dev), lab.to(dev)).backward()
    opt.step()
    torch.cuda.synchronize()
    num = den = 0.0
    before = dict(ref.named_parameters())
    for n, p in gref.named_parameters():
        num += (gp[n].detach().cpu().double() - p.detach()).pow(2).sum().item()
        den += (p.detach() - before[n].detach().double()).pow(2).sum().item()
    assert den > 0 and (num / den) ** 0.5 < 1e-2, (num, den)


def test_hip_sgd_checkpoint_loads_into_torch_sgd(dev, tmp_path, monkeypatch):
    from rgbx_semantic_segmentation_amd.engine.engine import Engine
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    ref, model = _pair(dev)
    model.eval()
    opt = _fused(model)
    rgb, x, lab = _batch(seed=4)
    for _ in range(2):
        model(rgb.to(dev), x.to(dev), lab.to(dev)).backward()
        opt.step()
    with Engine(argv=[]) as e:
        e.register_state(model=model, optimizer=opt)
        e.update_iteration(7, 2)
        e.save_and_link_checkpoint(str(tmp_path / "ck"), str(tmp_path / "log"), str(tmp_path / "log_last"))
    sd = torch.load(tmp_path / "ck" / "epoch-7.pth", weights_only=True)
    assert set(sd) == {"model", "optimizer", "epoch", "iteration"}
    ref2 = RefModel(CMXConfig(backbone=BACKBONE, num_classes=K))
    ref2.load_state_dict(sd["model"], strict=True)
    opt_t = _torch_opt(ref2)
    opt_t.load_state_dict(sd["optimizer"])
    bt, bg = _buffers(opt_t, ref2), _gpu_buffers(opt, model)
    assert set(bt) == set(bg)
    for n in bt:
        assert torch.equal(bt[n], bg[n]) and bt[n].abs().max() > 0, n
    for grp in opt_t.param_groups:
        assert grp["momentum"] == MOMENTUM and grp["lr"] == LR
    assert opt_t.param_groups[0]["weight_decay"] == WD and opt_t.param_groups[1]["weight_decay"] == 0.0
    gp = dict(model.named_parameters())
    for n, p in ref2.named_parameters():
        assert torch.equal(p.detach(), gp[n].detach().cpu())


# ------------------------------------------------------------------ 6. HIP graph
def test_captured_sgd_step_follows_the_lr(dev):
    _, model = _pair(dev, dtype="bfloat16")
    model.eval()
    opt = _fused(model)
    st = model.store
    rgb, x, lab = _batch()
    model(rgb.to(dev), x.to(dev), lab.to(dev)).backward()          # one eager backward: the gradients
    torch.cuda.synchronize()
    start = (st.flat.clone(), st.shadow.clone())
    lrs = (1e-2, 5e-3, 2e-2)

    def reset():
        st.flat.copy_(start[0])
        st.shadow.copy_(start[1])
        opt.momentum_buffer.zero_()

    def set_lr(lr):
        for grp in opt.param_groups:
            grp["lr"] = lr

    def state():
        torch.cuda.synchronize()
        return st.flat.clone(), opt.momentum_buffer.clone(), st.shadow.clone()

    for lr in lrs:
        set_lr(lr)
        opt.step()
    eager = state()
    assert not torch.equal(eager[0], start[0])
    reset()
    gc.collect()                       # no pinned-host frees of earlier tests inside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        opt.step()
    torch.cuda.synchronize()
    assert torch.equal(st.flat, start[0])                  # the capture itself ran nothing
    for lr in lrs:
        set_lr(lr)
        graph.replay()
    replayed = state()
    for a, b, what in zip(replayed, eager, ("p", "buf", "shadow")):
        assert torch.equal(a.view(torch.int32 if a.dtype == torch.float32 else torch.int16),
                           b.view(torch.int32 if b.dtype == torch.float32 else torch.int16)), what


# ------------------------------------------------------------------ 7. GradScaler, bf16 shadow
def test_grad_scaler_skips_then_steps_fused_sgd(dev):
    from rgbx_semantic_segmentation_amd.optim import GradScaler
    _, model = _pair(dev, dtype="bfloat16")
    model.eval()
    opt = _fused(model)
    st = model.store
    sc = GradScaler(init_scale=2.0 ** 10, device=dev)
    rgb, x, lab = (t.to(dev) for t in _batch())
    sc.scale(model(rgb, x, lab)).backward()
    sc.step(opt)
    sc.update()                                            # a clean step: buf is no longer zero
    torch.cuda.synchronize()
    assert sc.get_scale() == 2.0 ** 10 and opt.momentum_buffer.abs().max().item() > 0
    sc.scale(model(rgb, x, lab)).backward()
    sl = st.slot(opt._order[0])                            # one element of a grouped (decay) parameter
    assert sl.decay and not sl.frozen
    st.grad[sl.offset + 7] = float("inf")
    before = [t.clone() for t in (st.flat, opt.momentum_buffer, st.shadow)]
    sc.step(opt)
    sc.update()
    torch.cuda.synchronize()
    for t, was in zip((st.flat, opt.momentum_buffer, st.shadow), before):
        idt = torch.int32 if t.dtype == torch.float32 else torch.int16
        assert torch.equal(t.view(idt), was.view(idt))
    assert sc.get_scale() == 2.0 ** 9
    sc.scale(model(rgb, x, lab)).backward()                # the backward overwrites the inf
    sc.step(opt)
    sc.update()
    torch.cuda.synchronize()
    assert sc.get_scale() == 2.0 ** 9
    assert (st.flat - before[0]).norm().item() > 0 and bool(torch.isfinite(st.flat).all())
    assert torch.equal(st.shadow, st.flat.to(torch.bfloat16))


# ------------------------------------------------------------------ 8. train.main
def test_train_main_sgdm_and_resume(dev, tmp_path, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    import train
    base = ["--backbone", "mit_b0", "--num-classes", "9", "--height", "96", "--width", "128", "--batch-size", "2",
            "--niters-per-epoch", "4", "--warm-up-epoch", "0", "--optimizer", "SGDM", "--lr", "1e-2",
            "--compute-dtype", "float32", "--checkpoint-dir", str(tmp_path)]
    l1 = train.main(base + ["--nepochs", "1"])
    assert l1 == l1 and 0 < l1 < float("inf")
    ck = tmp_path / "epoch-1.pth"
    sd = torch.load(ck, weights_only=True)
    assert sd["epoch"] == 1 and sd["iteration"] == 3
    groups = sd["optimizer"]["param_groups"]
    assert len(groups) == 2 and all(g["momentum"] == 0.9 for g in groups)
    grouped = groups[0]["params"] + groups[1]["params"]
    assert len(grouped) > 0 and set(sd["optimizer"]["state"]) == set(grouped)
    for i in grouped:
        buf = sd["optimizer"]["state"][i]["momentum_buffer"]
        assert bool(torch.isfinite(buf).all()), i
    assert any(sd["optimizer"]["state"][i]["momentum_buffer"].abs().max() > 0 for i in grouped)
    l2 = train.main(base + ["--nepochs", "2", "-c", str(ck)])
    assert l2 == l2 and 0 < l2 < float("inf")
    assert (tmp_path / "epoch-2.pth").exists()
