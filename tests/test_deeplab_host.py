"""DeepLabV3Plus decode head, host side (no GPU): construction, keys, initialisation, the weight decay split, the
auxiliary head's default, train.py's flags, the new header's binding table and the MAC count."""
import os
import sys

import pytest
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from rgbx_semantic_segmentation_amd.models.builder import PE1_KPAD, EncoderDecoder, backward_segment  # noqa: E402
from rgbx_semantic_segmentation_amd.models.decoders.deeplabv3plus import DeepLabV3Plus  # noqa: E402
from rgbx_semantic_segmentation_amd.models.decoders.fcnhead import FCNHead  # noqa: E402
from rgbx_semantic_segmentation_amd.params import ParamStore  # noqa: E402
from deeplab_ref import DeepLabV3PlusRef, ref_model  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 9
ENTRY_POINTS = ("cmx_aspp_conv_fwd", "cmx_aspp_conv_dgrad", "cmx_aspp_conv_wgrad_workspace", "cmx_aspp_conv_wgrad",
                "cmx_upcat_ac_fwd", "cmx_upcat_ac_bwd")


def test_decoder_builds_with_the_aux_head_by_default():
    torch.manual_seed(0)
    m = EncoderDecoder(dict(backbone="mit_b0", decoder="DeepLabV3Plus", num_classes=K))
    h = m.decode_head
    assert isinstance(h, DeepLabV3Plus) and h.dropout_ratio == 0
    want = DeepLabV3PlusRef(m.channels, K).state_dict()
    got = h.state_dict()
    assert set(got) == set(want) and len(got) == 52
    assert all(got[n].shape == want[n].shape for n in want)
    assert h.block[0].weight.shape == (256, 304, 3, 3) and h.low_level[0].weight.shape == (48, 32, 3, 3)
    assert h.aspp.b1.block[0].weight.shape == (256, 256, 3, 3) and h.aspp.b3.block[0].dilation == (36, 36)
    assert h.block[4].weight.shape == (K, 256, 1, 1) and h.aspp.project[3].p == 0.5 and h.block[3].p == 0.1
    assert isinstance(m.aux_head, FCNHead) and m.aux_index == 2 and m.aux_rate == 0.4
    off = EncoderDecoder(dict(backbone="mit_b0", decoder="DeepLabV3Plus", num_classes=K, aux_head=False))
    assert off.aux_head is None
    assert EncoderDecoder(dict(backbone="mit_b0")).aux_head is None              # other decoders: still off by default
    b2 = EncoderDecoder(dict(backbone="mit_b2", decoder="DeepLabV3Plus", num_classes=K, aux_head=False)).decode_head
    assert b2.aspp.b2.block[0].weight.shape == (256, 512, 3, 3) and b2.low_level[0].weight.shape == (48, 64, 3, 3)


def test_reference_constructor_and_strict_load():
    torch.manual_seed(0)
    head = DeepLabV3Plus([64, 128, 320, 512], 7, nn.BatchNorm2d)                 # the reference's positional order
    head.load_state_dict(DeepLabV3PlusRef([64, 128, 320, 512], 7).state_dict(), strict=True)
    for aux in (True, False):
        ref = ref_model("mit_b0", aux_head=aux, num_classes=K)
        m = EncoderDecoder(dict(backbone="mit_b0", decoder="DeepLabV3Plus", num_classes=K, aux_head=aux))
        assert set(m.state_dict()) == set(ref.state_dict())
        m.load_state_dict(ref.state_dict(), strict=True)


@pytest.mark.parametrize("decoder", ["deeplabv3+", "UPernet", "mask2former"])
def test_reference_spellings_stay_refused(decoder):
    with pytest.raises(NotImplementedError) as e:
        EncoderDecoder(dict(decoder=decoder, backbone="mit_b0"))
    assert "MLPDecoder" in str(e.value) and "MLPDecoderpp" in str(e.value)
    assert ("DeepLabV3Plus" in str(e.value)) == (decoder == "deeplabv3+")


def test_init_weights_reaches_the_whole_head():
    torch.manual_seed(0)
    m = EncoderDecoder(dict(backbone="mit_b2", decoder="DeepLabV3Plus", num_classes=K, bn_eps=2e-3))
    convs = [c for c in m.decode_head.modules() if isinstance(c, nn.Conv2d)]
    bns = [b for b in m.decode_head.modules() if isinstance(b, nn.BatchNorm2d)]
    assert len(convs) == 9 and len(bns) == 8
    for conv in convs:
        fan_in = conv.weight.shape[1] * conv.weight.shape[2] * conv.weight.shape[3]
        if conv.weight.numel() >= 10000:                 # enough samples for a 10 % estimate of the spread
            assert abs(conv.weight.std().item() / (2.0 / fan_in) ** 0.5 - 1) < 0.1, conv
    for bn in bns:
        assert bn.eps == 2e-3 and bn.momentum == 0.1
        assert bool((bn.weight == 1).all()) and bool((bn.bias == 0).all())


def test_weight_decay_split_and_segments():
    m = EncoderDecoder(dict(backbone="mit_b0", decoder="DeepLabV3Plus", num_classes=K))
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
    assert len(seen) == 9 + 3 + 2 * 8 and len(conv_w) == 9            # conv weights, three biases, BN affine pairs
    seg0 = [b for sid, a, b in st.segments if sid == 0][0]
    assert all(st.slots[n].offset < seg0 for n in seen)


def test_train_parser_and_criterion_check():
    import train
    p = train.build_parser()
    a = p.parse_args(["--decoder", "DeepLabV3Plus"])
    assert a.decoder == "DeepLabV3Plus" and a.aux_head is False and a.no_aux_head is False
    assert train.effective_aux_head(a) is True
    b = p.parse_args(["--decoder", "DeepLabV3Plus", "--no-aux-head"])
    assert b.no_aux_head is True and train.effective_aux_head(b) is False
    assert train.effective_aux_head(p.parse_args([])) is False
    assert train.effective_aux_head(p.parse_args(["--aux-head"])) is True
    assert isinstance(train.build_criterion(a), nn.CrossEntropyLoss)
    with pytest.raises(NotImplementedError, match="DiceCELoss with aux_head.*aux_head=False"):
        train.build_criterion(p.parse_args(["--decoder", "DeepLabV3Plus", "--dice-alpha", "0.5"]))
    from rgbx_semantic_segmentation_amd.utils.loss_opr import DiceCELoss
    crit = train.build_criterion(p.parse_args(["--decoder", "DeepLabV3Plus", "--no-aux-head", "--dice-alpha", "0.5"]))
    assert isinstance(crit, DiceCELoss)
    for extra in (["--criterion", "ProbOhemCrossEntropy2d"], ["--criterion", "CE_Focal"]):
        with pytest.raises(NotImplementedError, match="aux_head=False"):
            train.build_criterion(p.parse_args(["--decoder", "DeepLabV3Plus"] + extra))
        train.build_criterion(p.parse_args(["--decoder", "DeepLabV3Plus", "--no-aux-head"] + extra))
    with pytest.raises(NotImplementedError, match="aux_head=False"):
        EncoderDecoder(dict(backbone="mit_b0", decoder="DeepLabV3Plus"), criterion=crit)
    EncoderDecoder(dict(backbone="mit_b0", decoder="DeepLabV3Plus", aux_head=False), criterion=crit)


def test_header_table_and_abi():
    from rgbx_semantic_segmentation_amd import _lib
    sigs = _lib.parse_header(os.path.join(ROOT, "include", "cmx_deeplab.h"))
    assert tuple(sigs) == ENTRY_POINTS == tuple(_lib.DEEPLAB_SIGNATURES)
    assert _lib.header_abi_version() == 7 and _lib.query("cmx_abi_version") == 7
    tables = (_lib.SIGNATURES, _lib.OHEM_SIGNATURES, _lib.EASPP_SIGNATURES, _lib.FCN_SIGNATURES)
    for name in sigs:
        assert _lib.DEEPLAB_SIGNATURES[name].kinds == sigs[name].kinds
        assert not any(name in t for t in tables) and getattr(_lib.LIB, name) is not None
    kinds = sigs["cmx_aspp_conv_fwd"].kinds
    assert len(kinds) == 19 and kinds[:7] == (_lib.POINTER,) * 7 and kinds[-1] == _lib.STREAM
    assert set(kinds[7:-1]) == {_lib.SCALAR}
    assert sigs["cmx_upcat_ac_bwd"].kinds == (_lib.POINTER,) * 3 + (_lib.SCALAR,) * 8 + (_lib.STREAM,)
    # the size query launches nothing.  Rows per chunk: 128 * min(16, Cin/64 * Cout/64), at most 8 chunks
    q = lambda *a: _lib.query("cmx_aspp_conv_wgrad_workspace", *a)
    assert q(2, 15, 20, 512, 256) == 0                                   # the training shape: one chunk, no partials
    assert q(2, 14, 26, 64, 128) == 3 * 3 * 128 * 9 * 64 * 4             # 728 rows in chunks of 256
    assert q(3, 13, 25, 128, 192) == 3 * 2 * 192 * 9 * 128 * 4           # 975 rows in chunks of 768
    assert q(2, 120, 160, 64, 64) == 3 * 8 * 64 * 9 * 64 * 4             # capped at 8 chunks
    for refused in ((0, 15, 20, 512, 256), (2, 15, 20, 96, 256), (2, 15, 20, 512, 32), (2, 15, 20, 2048, 256),
                    (2, 0, 20, 512, 256)):
        assert q(*refused) == 0


def test_macs_hand_count():
    from rgbx_semantic_segmentation_amd import flops
    assert flops.forward_macs_per_image() == flops.forward_macs_per_image(decoder="MLPDecoder") == 78201854976
    # mit_b0 at 64 x 96, K = 9: stage-1 grid 16 x 24 of 32 channels, stage-4 grid 2 x 3 of 256
    N1, N4 = 16 * 24, 2 * 3
    head = (N4 * 256 * 256                # aspp.b0
            + 3 * N4 * 9 * 256 * 256      # aspp.b1 .. b3, every tap
            + 256 * 256                   # aspp.b4's 1x1 conv on the pooled pixel
            + N4 * 1280 * 256             # aspp.project
            + N1 * 9 * 32 * 48            # low_level
            + N1 * 9 * 304 * 256          # block[0]
            + N1 * 256 * 9)               # block[4]
    assert flops.deeplabv3plus_macs(N1, 32, N4, 256, 9) == head
    kw = dict(backbone="mit_b0", H=64, W=96, K=9)
    mlp_head = sum(n * c * 512 for n, c in ((384, 32), (96, 64), (24, 160), (6, 256))) + N1 * 4 * 512 * 512 + N1 * 512 * 9
    assert flops.forward_macs_per_image(decoder="DeepLabV3Plus", **kw) - head \
        == flops.forward_macs_per_image(**kw) - mlp_head
