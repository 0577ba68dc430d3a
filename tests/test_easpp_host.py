"""The mit_b*_w_ef_aspp backbones on the host (no GPU): the builder accepts the six names, the neck's state_dict is
the reference's (tests/easpp_ref.py restates it under the reference's names), its init, its place in the weight-decay
grouping and the backward segments, the work it adds to the FLOP count, and its C-ABI header part."""
import math
import os

import pytest
import torch
import torch.nn as nn

from easpp_ref import EASPPRef, ref_model
from rgbx_semantic_segmentation_amd.models.builder import EncoderDecoder, PE1_KPAD, backward_segment
from rgbx_semantic_segmentation_amd.models.encoders.dual_segformer import MIT_SPECS
from rgbx_semantic_segmentation_amd.params import ParamStore

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NECK = "backbone.single_aspp."
PLAIN = ("mit_b0", "mit_b1", "mit_b2", "mit_b3", "mit_b4", "mit_b5")


def _model(backbone="mit_b0_w_ef_aspp", **kw):
    torch.manual_seed(0)
    return EncoderDecoder(dict(backbone=backbone, num_classes=9, **kw))


def test_state_dict_is_the_oracles_with_the_restated_neck():
    m, plain = _model(), _model("mit_b0")
    ref = ref_model("mit_b0", num_classes=9)
    sd, rsd = m.state_dict(), ref.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v.shape) for k, v in rsd.items()}
    neck = [k for k in sd if k.startswith(NECK)]
    assert len(neck) == 108 and len(sd) == len(plain.state_dict()) + 108
    assert set(sd) - set(neck) == set(plain.state_dict())
    count = lambda mod: sum(p.numel() for p in mod.parameters())
    assert count(m) - count(plain) == count(EASPPRef(256)) == count(m.backbone.single_aspp)
    m.load_state_dict(rsd, strict=True)


def test_size_at_512_channels():
    neck = EASPPRef(512)
    convs = [x for x in neck.modules() if isinstance(x, nn.Conv2d)]
    bns = [x for x in neck.modules() if isinstance(x, nn.BatchNorm2d)]
    assert (len(convs), len(bns)) == (18, 18) and all(c.bias is None for c in convs)
    assert sum(p.numel() for p in neck.parameters()) == 1401856 and len(neck.state_dict()) == 108
    ours = _model("mit_b2_w_ef_aspp").backbone.single_aspp
    assert {k: tuple(v.shape) for k, v in ours.state_dict().items()} == \
        {k: tuple(v.shape) for k, v in neck.state_dict().items()}


@pytest.mark.parametrize("norm_layer", [nn.BatchNorm2d, nn.SyncBatchNorm])
def test_init_and_norm_types(norm_layer):
    torch.manual_seed(0)
    m = EncoderDecoder(dict(backbone="mit_b0_w_ef_aspp", num_classes=9), norm_layer=norm_layer)
    neck = m.backbone.single_aspp
    convs = [x for x in neck.modules() if isinstance(x, nn.Conv2d)]
    bns = [x for x in neck.modules() if isinstance(x, nn.modules.batchnorm._BatchNorm)]
    assert len(convs) == 18 and len(bns) == 18
    for c in convs:
        fan_out = c.kernel_size[0] * c.kernel_size[1] * c.out_channels
        assert abs(c.weight.std().item() / math.sqrt(2.0 / fan_out) - 1) < 0.1, c
        assert c.bias is None
    for b in bns:
        assert type(b) is nn.BatchNorm2d and (b.eps, b.momentum) == (1e-5, 0.1)
        assert bool((b.weight == 1).all()) and bool((b.bias == 0).all())
    d = neck.project[3]
    assert type(d) is nn.Dropout and d.p == 0.5
    rates = [neck.branch1[1].block[0].dilation, neck.branch2[2].block[0].dilation, neck.branch3[3].block[0].dilation]
    assert rates == [(12, 12), (24, 24), (36, 36)]
    assert neck.branch2[1].block[0].padding == (24, 24)


def test_weight_decay_segments_and_flags():
    """Conv weights decay, BN affine parameters do not, nothing is frozen, the per-64-element flags of the flat
    buffer agree, and every neck parameter completes in backward segment 0 (with stage 4 and the decode head)."""
    m = _model()
    st = ParamStore(m, "cpu", torch.float32, conv_pad={"backbone.patch_embed1.proj.weight": PE1_KPAD,
                                                       "backbone.extra_patch_embed1.proj.weight": PE1_KPAD},
                    segment_of=backward_segment)
    owner = {NECK + n + ".weight": mod for n, mod in m.backbone.single_aspp.named_modules()}
    owner.update({NECK + n + ".bias": mod for n, mod in m.backbone.single_aspp.named_modules()})
    seen = 0
    for n, s in st.slots.items():
        if not n.startswith(NECK):
            continue
        seen += 1
        is_conv = isinstance(owner[n], nn.Conv2d)
        assert s.decay == is_conv and not s.frozen and s.count == 1, n
        assert backward_segment(n) == 0, n
        flags = st.decay64[s.offset // 64:(s.offset + s.stride * s.count + 63) // 64]
        assert bool((flags == (1 if is_conv else 0)).all()), n
        if is_conv and owner[n].kernel_size == (3, 3):
            assert s.kind == "conv_taps" and s.storage_shape == (64, 3, 3, 64), n
    assert seen == 18 + 2 * 18
    seg0 = [b for sid, a, b in st.segments if sid == 0][0]
    assert all(s.offset < seg0 for n, s in st.slots.items() if n.startswith(NECK))


@pytest.mark.parametrize("name", PLAIN)
def test_all_six_names_build(name):
    """Each new name builds with the plain name's depths and with channels from embed_dims (the reference's
    hard-coded 768 for b4 / b5 cannot run); the plain name still gives the oracle's state_dict, key for key, and the
    new one exactly those plus the neck's 108."""
    from oracle.cmx_ref import CMXConfig, EncoderDecoder as OracleModel
    plain = MIT_SPECS[name]
    assert MIT_SPECS[name + "_w_ef_aspp"]["embed_dims"] == plain["embed_dims"]
    m = _model(name + "_w_ef_aspp")
    assert m.channels == plain["embed_dims"] and m.backbone.depths == plain["depths"]
    neck = m.backbone.single_aspp
    C4 = plain["embed_dims"][3]
    assert neck.project[0].out_channels == C4 and neck.project[0].in_channels == 5 * 256
    assert [c.in_channels for c in (neck.input_conv[0], neck.branch1[0][0], neck.branch2[0][0], neck.branch3[0][0],
                                    neck.img_pooling.gap[1])] == [C4] * 5
    assert type(m.backbone).__name__ == name + "_w_ef_aspp"
    base = _model(name)
    assert not hasattr(base.backbone, "single_aspp")
    shapes = lambda mod: {k: tuple(v.shape) for k, v in mod.state_dict().items()}
    want = shapes(OracleModel(CMXConfig(backbone=name, num_classes=9)))
    assert list(base.state_dict()) == list(want) and shapes(base) == want
    ours = shapes(m)
    assert {k: v for k, v in ours.items() if not k.startswith(NECK)} == want
    assert len(ours) == len(want) + 108


@pytest.mark.parametrize("name", ["mit_b2_w_aspp", "swin_s", "mit_b6_w_ef_aspp"])
def test_other_names_still_refused(name):
    with pytest.raises(NotImplementedError):
        EncoderDecoder(dict(backbone=name))


def test_training_with_one_image_is_refused():
    neck = _model().backbone.single_aspp
    with pytest.raises(ValueError):
        neck.run(None, torch.zeros(6, 256), 1, 2, 3, True)


def test_mask_state_is_not_made_inside_a_capture(monkeypatch):
    """The device step counter of the random dropout mask made inside a graph capture would be zeroed again by every
    replay (the same mask each time): the first random draw under a capture raises before it allocates anything."""
    neck = _model().backbone.single_aspp
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="eager"):
        neck.dropout_scale(12 * 256, "cuda")
    assert "_mask_state" not in neck.__dict__
    assert neck.dropout_scale(12, "cpu", mask=torch.ones(12)).tolist() == [2.0] * 12        # a forced mask needs none


@pytest.mark.parametrize("name,H,W", [("mit_b2", 480, 640), ("mit_b0", 64, 96), ("mit_b0", 64, 416)])
def test_flops_grow_by_the_necks_macs(name, H, W):
    from rgbx_semantic_segmentation_amd.flops import forward_macs_per_image as f
    from rgbx_semantic_segmentation_amd.floor import step_work
    C4 = MIT_SPECS[name]["embed_dims"][3]
    hw = (H // 32) * (W // 32)
    want = hw * (C4 * 448 + 9 * 9 * 64 * 64 + 3 * 64 * 256 + 1280 * C4) + C4 * 256
    assert f(name + "_w_ef_aspp", H=H, W=W) - f(name, H=H, W=W) == want
    a, b = step_work(backbone=name + "_w_ef_aspp", H=H, W=W), step_work(backbone=name, H=H, W=W)
    assert "easpp" in a and "easpp" not in b
    # the executed count: forward + input gradient + weight gradient of every product of the formula
    grown = sum(v[0] for v in a.values()) - sum(v[0] for v in b.values())
    assert grown == pytest.approx(2 * 3 * 2 * want, rel=1e-9)       # B = 2 images, 3 passes, 2 FLOP per MAC


def test_header_part_parses_and_symbols_resolve():
    from rgbx_semantic_segmentation_amd import _lib
    assert _lib.header_abi_version() == 7 and _lib.query("cmx_abi_version") == 7
    sigs = _lib.parse_header(os.path.join(ROOT, "include", "cmx_easpp.h"))
    want = {"cmx_easpp_conv_fwd": 20, "cmx_easpp_conv_dgrad": 20, "cmx_easpp_conv_wgrad_workspace": 3,
            "cmx_easpp_conv_wgrad": 21, "cmx_easpp_concat_fwd": 11, "cmx_easpp_concat_bwd": 11,
            "cmx_easpp_pool_bwd": 9, "cmx_easpp_dropout_mask": 6}
    assert {n: len(s[1]) for n, s in sigs.items()} == want
    assert tuple(sigs) == tuple(_lib.EASPP_SIGNATURES)
    assert not set(sigs) & (set(_lib.SIGNATURES) | set(_lib.OHEM_SIGNATURES))
    for name in sigs:
        assert getattr(_lib.LIB, name) is not None
        assert _lib.EASPP_SIGNATURES[name].kinds == sigs[name].kinds
        if name != "cmx_easpp_conv_wgrad_workspace":
            assert sigs[name].kinds[-1] == _lib.STREAM
    # the size query launches nothing: 128-row chunks, no workspace for a single chunk
    assert _lib.query("cmx_easpp_conv_wgrad_workspace", 1, 2, 3) == 0
    assert _lib.query("cmx_easpp_conv_wgrad_workspace", 2, 15, 20) == 3 * 5 * 64 * 9 * 64 * 4
    with pytest.raises(TypeError):
        _lib.marshal("cmx_easpp_dropout_mask", (None, 1, 0.5))
