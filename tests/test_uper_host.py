"""UPerHead decode head, host side (no GPU): the restatement against outputs recorded from the reference's own class,
construction, keys, initialisation, the weight decay split, the auxiliary head's default, train.py's flags, the new
header's binding table and the MAC count."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from rgbx_semantic_segmentation_amd.models.builder import PE1_KPAD, EncoderDecoder, backward_segment  # noqa: E402
from rgbx_semantic_segmentation_amd.models.decoders.UPernet import PPM, UPerHead  # noqa: E402
from rgbx_semantic_segmentation_amd.models.decoders.fcnhead import FCNHead  # noqa: E402
from rgbx_semantic_segmentation_amd.params import ParamStore  # noqa: E402
from uper_ref import UPerHeadRef, ref_model  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 9
ENTRY_POINTS = ("cmx_ppm_pool_fwd", "cmx_ppm_pool_bwd", "cmx_upcat_multi_fwd", "cmx_upcat_multi_bwd", "cmx_up_add_fwd",
                "cmx_conv_flip_weight")


def test_restatement_reproduces_the_reference_forward():
    """tests/golden/uperhead_fwd.npz holds what the reference's own UPerHead computed on the CPU (fp32) in eval and in
    train mode; UPerHeadRef with the same weights must give the same values to fp32 rounding.  The outputs are O(1)
    sums of a few thousand fp32 products whose order differs between the two only where torch picks another
    convolution algorithm: 1e-5 absolute is about 50 ulp at that magnitude."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "uperhead_fwd.npz"))
    feats = [torch.from_numpy(z[f"feat{i}"]) for i in range(4)]
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd.")}
    assert len(sd) == 86
    head = UPerHeadRef([f.shape[1] for f in feats], num_classes=z["out_eval"].shape[1], channels=16)
    head.load_state_dict(sd, strict=True)
    # and the product's module takes the same checkpoint strictly (names and shapes)
    UPerHead([f.shape[1] for f in feats], z["out_eval"].shape[1], 16).load_state_dict(sd, strict=True)
    with torch.no_grad():
        for mode, key in ((False, "out_eval"), (True, "out_train")):
            got = head.train(mode)(feats)
            want = torch.from_numpy(z[key])
            assert got.shape == want.shape == (2, 5, 12, 10)
            err = (got - want).abs().max().item()
            print(key, "max abs difference", err, "of", want.abs().max().item())
            assert err <= 1e-5, (key, err)
    # fp64 agrees with the recorded fp32 values to fp32 accuracy as well: any float dtype (the weights again: the
    # train-mode run above moved the running statistics)
    head.load_state_dict(sd, strict=True)
    with torch.no_grad():
        got = head.double().eval()([f.double() for f in feats])
    assert (got - torch.from_numpy(z["out_eval"]).double()).abs().max().item() <= 1e-5


def test_decoder_builds_with_the_aux_head_by_default():
    torch.manual_seed(0)
    m = EncoderDecoder(dict(backbone="mit_b0", decoder="UPerHead", num_classes=K))
    h = m.decode_head
    assert isinstance(h, UPerHead) and isinstance(h.psp_modules, PPM) and h.dropout_ratio == 0 and h.embed_dim == 512
    want = UPerHeadRef(m.channels, K).state_dict()
    got = h.state_dict()
    assert set(got) == set(want) and len(got) == 86 == 12 * 7 + 2
    assert all(got[n].shape == want[n].shape for n in want)
    assert h.bottleneck[0].weight.shape == (512, 256 + 4 * 512, 3, 3)
    assert h.fpn_bottleneck[0].weight.shape == (512, 2048, 3, 3) and h.conv_seg.weight.shape == (K, 512, 1, 1)
    assert [s[1].weight.shape for s in h.psp_modules] == [(512, 256, 1, 1)] * 4
    assert [s[0].weight.shape[1] for s in h.lateral_convs] == [32, 64, 160]
    assert all(c.bias is not None for c in h.modules() if isinstance(c, nn.Conv2d))
    assert isinstance(m.aux_head, FCNHead) and m.aux_index == 2 and m.aux_rate == 0.4
    off = EncoderDecoder(dict(backbone="mit_b0", decoder="UPerHead", num_classes=K, aux_head=False))
    assert off.aux_head is None
    assert EncoderDecoder(dict(backbone="mit_b0")).aux_head is None              # other decoders: unchanged
    assert EncoderDecoder(dict(backbone="mit_b0", decoder="FCNHead")).aux_head is None
    assert EncoderDecoder(dict(backbone="mit_b0", decoder="DeepLabV3Plus")).aux_head is not None
    assert type(EncoderDecoder(dict(backbone="mit_b0")).decode_head).__module__.endswith("decoders.MLPDecoder")


def test_reference_constructor_and_strict_load():
    torch.manual_seed(0)
    head = UPerHead([64, 128, 320, 512], 7, 512, (1, 2, 3, 6), nn.BatchNorm2d)    # the reference's positional order
    head.load_state_dict(UPerHeadRef([64, 128, 320, 512], 7).state_dict(), strict=True)
    UPerHeadRef([64, 128, 320, 512], 7).load_state_dict(head.state_dict(), strict=True)
    for aux in (True, False):
        ref = ref_model("mit_b0", aux_head=aux, num_classes=K)
        m = EncoderDecoder(dict(backbone="mit_b0", decoder="UPerHead", num_classes=K, aux_head=aux))
        assert set(m.state_dict()) == set(ref.state_dict())
        m.load_state_dict(ref.state_dict(), strict=True)
        ref.load_state_dict(m.state_dict(), strict=True)


def test_constructor_refusals():
    for scales in ((1, 2, 3), (1, 2, 3, 6, 8), (1, 2, 3, 9), (0, 2, 3, 6)):
        with pytest.raises(NotImplementedError, match="pool_scales"):
            UPerHead([32, 64, 160, 256], K, pool_scales=scales)
    with pytest.raises(NotImplementedError, match="align_corners"):
        UPerHead([32, 64, 160, 256], K, align_corners=True)
    UPerHead([32, 64, 160, 256], K, channels=64, pool_scales=(1, 2, 4, 8))


def test_the_reference_spelling_stays_refused_with_a_hint():
    with pytest.raises(NotImplementedError) as e:
        EncoderDecoder(dict(decoder="UPernet", backbone="mit_b0"))
    msg = str(e.value)
    assert "MLPDecoder" in msg and "MLPDecoderpp" in msg and "decoder='UPerHead'" in msg
    assert "DeepLabV3Plus" not in msg
    with pytest.raises(NotImplementedError) as e:
        EncoderDecoder(dict(decoder="mask2former", backbone="mit_b0"))
    assert "UPerHead" not in str(e.value)


def test_init_weights_reaches_the_whole_head():
    torch.manual_seed(0)
    m = EncoderDecoder(dict(backbone="mit_b2", decoder="UPerHead", num_classes=K, bn_eps=2e-3))
    convs = [c for c in m.decode_head.modules() if isinstance(c, nn.Conv2d)]
    bns = [b for b in m.decode_head.modules() if isinstance(b, nn.BatchNorm2d)]
    assert len(convs) == 13 and len(bns) == 12
    for conv in convs:
        fan_in = conv.weight.shape[1] * conv.weight.shape[2] * conv.weight.shape[3]
        if conv.weight.numel() >= 10000:                 # enough samples for a 10 % estimate of the spread
            assert abs(conv.weight.std().item() / (2.0 / fan_in) ** 0.5 - 1) < 0.1, conv
    for bn in bns:
        assert bn.eps == 2e-3 and bn.momentum == 0.1
        assert bool((bn.weight == 1).all()) and bool((bn.bias == 0).all())


def test_weight_decay_split_and_segments():
    m = EncoderDecoder(dict(backbone="mit_b0", decoder="UPerHead", num_classes=K))
    st = ParamStore(m, "cpu", torch.float32, conv_pad={"backbone.patch_embed1.proj.weight": PE1_KPAD,
                                                       "backbone.extra_patch_embed1.proj.weight": PE1_KPAD},
                    segment_of=backward_segment)
    conv_w = {"decode_head." + n + ".weight" for n, c in m.decode_head.named_modules() if isinstance(c, nn.Conv2d)}
    seen = set()
    for n, s in st.slots.items():
        if not n.startswith("decode_head."):
            continue
        seen.add(n)
        assert s.decay == (n in conv_w) and not s.frozen and backward_segment(n) == 0, n
        if n in conv_w and m.decode_head.get_parameter(n[len("decode_head."):]).shape[2] == 3:
            assert s.kind == "conv_taps" and s.storage_shape[1:3] == (3, 3), n
    assert len(seen) == 13 + 13 + 2 * 12 and len(conv_w) == 13       # conv weights, their biases, BN affine pairs
    seg0 = [b for sid, a, b in st.segments if sid == 0][0]
    assert all(st.slots[n].offset < seg0 for n in seen)


def test_train_parser_and_criterion_check():
    import train
    p = train.build_parser()
    a = p.parse_args(["--decoder", "UPerHead"])
    assert a.decoder == "UPerHead" and a.aux_head is False and a.no_aux_head is False
    assert train.effective_aux_head(a) is True
    b = p.parse_args(["--decoder", "UPerHead", "--no-aux-head"])
    assert b.no_aux_head is True and train.effective_aux_head(b) is False
    assert train.effective_aux_head(p.parse_args([])) is False
    assert train.effective_aux_head(p.parse_args(["--decoder", "DeepLabV3Plus"])) is True
    with pytest.raises(SystemExit):
        p.parse_args(["--decoder", "UPernet"])
    assert isinstance(train.build_criterion(a), nn.CrossEntropyLoss)
    with pytest.raises(NotImplementedError, match="DiceCELoss with aux_head.*aux_head=False"):
        train.build_criterion(p.parse_args(["--decoder", "UPerHead", "--dice-alpha", "0.5"]))
    from rgbx_semantic_segmentation_amd.utils.loss_opr import DiceCELoss
    crit = train.build_criterion(p.parse_args(["--decoder", "UPerHead", "--no-aux-head", "--dice-alpha", "0.5"]))
    assert isinstance(crit, DiceCELoss)
    with pytest.raises(NotImplementedError, match="DiceLoss with aux_head.*aux_head=False"):
        train.build_criterion(p.parse_args(["--decoder", "UPerHead", "--dice-alpha", "1"]))
    for extra in (["--criterion", "ProbOhemCrossEntropy2d"], ["--criterion", "CE_Focal"]):
        with pytest.raises(NotImplementedError, match="aux_head=False"):
            train.build_criterion(p.parse_args(["--decoder", "UPerHead"] + extra))
        train.build_criterion(p.parse_args(["--decoder", "UPerHead", "--no-aux-head"] + extra))
    with pytest.raises(NotImplementedError, match="aux_head=False"):
        EncoderDecoder(dict(backbone="mit_b0", decoder="UPerHead"), criterion=crit)
    EncoderDecoder(dict(backbone="mit_b0", decoder="UPerHead", aux_head=False), criterion=crit)


def test_header_table_and_abi():
    from rgbx_semantic_segmentation_amd import _lib
    sigs = _lib.parse_header(os.path.join(ROOT, "include", "cmx_uper.h"))
    assert tuple(sigs) == ENTRY_POINTS == tuple(_lib.UPER_SIGNATURES)
    assert _lib.header_abi_version() == 7 and _lib.query("cmx_abi_version") == 7
    assert len(_lib.SIGNATURES) == 130                                    # cmx_hip.h itself is untouched
    tables = (_lib.SIGNATURES, _lib.OHEM_SIGNATURES, _lib.EASPP_SIGNATURES, _lib.FCN_SIGNATURES,
              _lib.DEEPLAB_SIGNATURES, _lib.MLP_SIGNATURES)
    for name in sigs:
        assert _lib.UPER_SIGNATURES[name].kinds == sigs[name].kinds
        assert not any(name in t for t in tables) and getattr(_lib.LIB, name) is not None
        assert sigs[name].kinds[-1] == _lib.STREAM
    P, S = _lib.POINTER, _lib.SCALAR
    assert sigs["cmx_ppm_pool_fwd"].kinds == (P,) * 2 + (S,) * 9 + (_lib.STREAM,)
    assert sigs["cmx_ppm_pool_bwd"].kinds == (P, P, S, P) + (S,) * 9 + (_lib.STREAM,)
    assert sigs["cmx_upcat_multi_fwd"].kinds == (P,) * 6 + (S,) * 15 + (_lib.STREAM,)
    assert sigs["cmx_upcat_multi_bwd"].kinds == (P,) * 6 + (S,) * 15 + (_lib.STREAM,)
    assert sigs["cmx_up_add_fwd"].kinds == (P,) * 3 + (S,) * 7 + (_lib.STREAM,)
    assert sigs["cmx_conv_flip_weight"].kinds == (P,) * 2 + (S,) * 6 + (_lib.STREAM,)


def test_macs_match_the_issue_table():
    from rgbx_semantic_segmentation_amd import flops
    assert flops.forward_macs_per_image() == flops.forward_macs_per_image(decoder="MLPDecoder") == 78201854976
    # mit_b2 at 480 x 640, per image (the table is for two images, in GMAC)
    grids = [(120 * 160, 64), (60 * 80, 128), (30 * 40, 320), (15 * 20, 512)]
    Ch, Kc = 512, 40
    parts = {"fpn_bottleneck": 19200 * 9 * 2048 * Ch, "fpn0": 19200 * 9 * Ch * Ch, "fpn1": 4800 * 9 * Ch * Ch,
             "fpn2": 1200 * 9 * Ch * Ch, "bottleneck": 300 * 9 * 2560 * Ch,
             "small": (19200 * 64 + 4800 * 128 + 1200 * 320) * Ch + 50 * 512 * Ch + 19200 * Ch * Kc}
    for name, gmac2 in (("fpn_bottleneck", 362), ("fpn0", 91), ("fpn1", 23), ("fpn2", 6), ("bottleneck", 7),
                        ("small", 3)):
        assert round(2 * parts[name] / 1e9) == gmac2, name
    total = flops.uperhead_macs(grids, Kc)
    assert total == sum(parts.values())
    assert abs(2 * total / 1e12 - 0.49) < 0.005 and abs(6 * total / 1e12 - 1.5) < 0.03
    kw = dict(backbone="mit_b2", H=480, W=640, K=Kc)
    mlp_head = sum(n * c * 512 for n, c in grids) + 19200 * 4 * 512 * 512 + 19200 * 512 * Kc
    assert flops.forward_macs_per_image(decoder="UPerHead", **kw) - total == flops.forward_macs_per_image(**kw) - mlp_head
