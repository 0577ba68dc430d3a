"""The constructions of tests/adamw_cases.py hold on the CPU alone (no kernel): every case meets the moved
condition, an fp32 restatement of adamw_kernel's formula stays within the bound the GPU test asks of the
kernel, the frozen elements of the reference never move, the loss-scale restatement is torch's GradScaler,
the C-ABI declares and exports the six entry points without a revision bump, and their argument refusals
precede any launch.  Prints moved / bound and the restatement's err / bound of every case."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adamw_cases as ac  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sizes_are_the_grids_they_name():
    blocks = {name: -(-(n // 4) // 256) for name, (n, _) in ac.SIZES.items()}
    assert blocks == dict(n64=1, n1088=2, n64000_cap3=63, n64000=63, n131136=129, n131136_cap65=129)
    assert all(n % 64 == 0 for n, _ in ac.SIZES.values())
    # the cap of 65 leaves threads with only the unrolled loop and threads with only the tail
    nv, stride = 131136 // 4, 65 * 256
    # (thread i < nv - stride loops once and is done; thread i >= nv - stride never loops and takes the tail)
    assert stride < nv < 2 * stride and 0 < nv - stride < stride
    # the cap of 3: every thread loops ten times, the first 640 then take the tail
    nv, stride = 64000 // 4, 3 * 256
    assert nv // (2 * stride) == 10 and nv % (2 * stride) == 640 < stride
    assert ac.NF_N == 4194496 and ac.NF_N % 64 == 0
    fl = ac.flags(ac.NF_N)
    assert all(fl[e // 64] != 2 for e in ac.nf_positions(ac.NF_N)) and all(fl[e // 64] == 2 for e in ac.NF_FROZEN)
    assert ac.NF_FROZEN[0] < ac.NF_PASS <= ac.NF_FROZEN[1]


def test_inputs_hold_their_edge_values():
    for n, _ in ac.SIZES.values():
        p, gs, fe, m0, v0 = ac.inputs(n)
        frozen = fe == 2
        assert len(gs) == 4 and bool((v0 >= 0).all())
        for g in gs:
            assert g[5] == 0 and g[7] == 1e-30 and (g[7] * g[7]) == 0            # g^2 underflows in fp32
            assert bool(g[frozen].isnan().all()) and bool(torch.isfinite(g[~frozen]).all())
        assert (fe[:192:64].tolist()) == [1, 0, 2][:len(fe[:192:64])]
        for start in ac.STARTS:
            m, v, t = ac.start_state(n, start)
            assert bool((m[frozen] == ac.MV_FROZEN).all() and (v[frozen] == ac.MV_FROZEN).all())
            assert t == (0 if start == "fresh" else 9999)


@pytest.mark.parametrize("case", ac.CASES, ids=ac.case_id)
def test_moved_condition_and_restatement_within_the_bound(case):
    size, hyper, start, scale = case
    n = ac.SIZES[size][0]
    p, _, fe, _, _ = ac.inputs(n)
    live, frozen = fe != 2, fe == 2
    m, v, t0 = ac.start_state(n, start)
    ref = ac.reference(n, hyper, start, scale)
    got = ac.restate_kernel(p, ac.kernel_grads(n, scale), fe, hyper, m, v, t0, loss_scale=scale)
    assert len(ref) == len(got) == 4
    for it, (r, (pk, mk, vk, tk)) in enumerate(zip(ref, got)):
        assert r["step"] == tk == t0 + it + 1
        ratio = r["moved"] / r["bound_p"]
        line = f"{ac.case_id(case)} step {it}: moved / bound {ratio:.0f};"
        assert ratio >= ac.MOVED, (it, r["moved"], r["bound_p"])                 # the moved condition
        for name, a in (("p", pk), ("m", mk), ("v", vk)):
            err = (a.double() - r[name])[live].abs().max().item()
            line += f" {name} err / bound {err / r['bound_' + name]:.2f}"
            assert err <= r["bound_" + name], (it, name, err, r["bound_" + name])
        print(line)
        # the frozen elements: never in a group, so the reference holds the start there
        assert torch.equal(r["p"][frozen], p.double()[frozen])
        assert torch.equal(pk[frozen], p[frozen]) and bool((mk[frozen] == ac.MV_FROZEN).all())
        assert bool((vk[frozen] == ac.MV_FROZEN).all())
        assert bool(torch.isfinite(r["p"]).all() and torch.isfinite(pk).all())   # no NaN leaked from frozen g


def test_restatement_catches_the_fp32_one_minus_beta2():
    """1.f - 0.999f is 1.3e-5 (relative) off 0.001: v of the first step leaves its bound"""
    import numpy as np
    n = 1088
    p, gs, fe, _, _ = ac.inputs(n)
    live = fe != 2
    r = ac.reference(n, "default")[0]
    wrong = (np.float32(1.0) - np.float32(0.999)) * gs[0].numpy() * gs[0].numpy()
    err = (torch.from_numpy(wrong).double() - r["v"])[live].abs().max().item()
    assert err > 10 * r["bound_v"], (err, r["bound_v"])


# ------------------------------------------------------------------ the loss scale
def test_loss_scale_restatement_is_torchs_grad_scaler():
    s = ac.SCALE_START
    scale, tracker = s["scale"], 0
    want = ac.torch_scaler_sequence()
    assert len(want) == len(ac.SCALE_SEQUENCE) == 12
    seen = []
    for found, (ts, tt) in zip(ac.SCALE_SEQUENCE, want):
        scale, tracker, cleared = ac.loss_scale_update(scale, tracker, float(found), s["growth"], s["backoff"], s["interval"])
        assert (scale, tracker, cleared) == (ts, tt, 0.0), (found, scale, tracker, ts, tt)
        seen.append(scale)
    # the sequence backs off, grows after three clean steps, and backs off twice in a row
    assert seen == [1024, 1024, 512, 512, 512, 1024, 1024, 512, 256, 256, 256, 512]


# ------------------------------------------------------------------ the C-ABI
ENTRY_ARGS = dict(cmx_adamw_tickets=0, cmx_adamw_step=17, cmx_adamw_step_scaled=19, cmx_adamw_step_segment=19,
                  cmx_grad_nonfinite=5, cmx_loss_scale_update=7)


def test_header_declares_and_library_exports_the_adamw_family():
    from rgbx_semantic_segmentation_amd import _lib
    sigs = _lib.parse_header(os.path.join(ROOT, "include", "cmx_hip.h"))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in ENTRY_ARGS.items():
        assert name in sigs and hasattr(lib, name), name
        rt, argt = sigs[name]
        assert len(argt) == nargs, (name, len(argt))
        assert rt is (ctypes.c_size_t if name == "cmx_adamw_tickets" else ctypes.c_int32), name
    for name in ("cmx_adamw_step", "cmx_adamw_step_scaled", "cmx_adamw_step_segment"):
        argt = sigs[name][1]
        assert argt[7] is ctypes.c_int64                                           # n
        assert argt[10] is ctypes.c_double and argt[11] is ctypes.c_double         # beta1, beta2
        assert argt[12] is ctypes.c_float and argt[13] is ctypes.c_double          # eps, weight_decay
        assert argt[14] is ctypes.c_float                                          # grad_scale
    seg = sigs["cmx_adamw_step_segment"][1]
    assert seg[15] is ctypes.c_int32 and seg[16] is ctypes.c_int32                 # store_step, max_blocks
    assert sigs["cmx_grad_nonfinite"][1][1] is ctypes.c_int64
    assert lib.cmx_abi_version() == _lib.header_abi_version() == 7                 # unchanged
    assert _lib.query("cmx_adamw_tickets") == 1 + 4096


# fake non-null pointers: only ever handed to calls that validation refuses, so never dereferenced
_P, _G, _M, _V, _S, _D, _LR, _T, _F = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000, 0x8000, 0x9000


def _step_args(p=_P, g=_G, m=_M, v=_V, shadow=None, code=0, d=_D, n=64, lr=_LR, t=_T):
    return (p, g, m, v, shadow, code, d, n, lr, t, 0.9, 0.999, 1e-8, 0.01, 1.0)


REFUSALS = [("n = 63", dict(n=63), "shape"), ("shadow, dtype 0", dict(shadow=_S, code=0), "dtype"),
            ("shadow, dtype 3", dict(shadow=_S, code=3), "dtype")]
REFUSALS += [(f"{k} NULL", {k: None}, "arg") for k in ("p", "g", "m", "v", "d", "lr", "t")]
ENTRY_TAILS = {"cmx_adamw_step": (None, None), "cmx_adamw_step_scaled": (None, None, None, None),
               "cmx_adamw_step_segment": (1, 0, None, None)}


@pytest.mark.parametrize("entry", list(ENTRY_TAILS))
@pytest.mark.parametrize("what, kw, status", REFUSALS, ids=[r[0].replace(" ", "_") for r in REFUSALS])
def test_adamw_steps_refuse_before_launching(entry, what, kw, status):
    from rgbx_semantic_segmentation_amd import _lib
    want = {"shape": _lib.CMX_ERR_SHAPE, "dtype": _lib.CMX_ERR_DTYPE, "arg": _lib.CMX_ERR_ARG}[status]
    st = getattr(_lib.LIB, entry)(*_step_args(**kw), *ENTRY_TAILS[entry])
    assert st == want, (entry, what, st, _lib.last_error())
    assert "adamw" in _lib.last_error()


@pytest.mark.parametrize("what, args", [
    ("n % 4", (_G, 66, None, _F, None)),
    ("found_inf NULL", (_G, 64, None, None, None)),
    ("flags and n % 64", (_G, 68, _D, _F, None)),
])
def test_grad_nonfinite_refuses_before_launching(what, args):
    from rgbx_semantic_segmentation_amd import _lib
    st = _lib.LIB.cmx_grad_nonfinite(*args)
    assert st == _lib.CMX_ERR_SHAPE, (what, st, _lib.last_error())
    assert "grad_nonfinite" in _lib.last_error()
