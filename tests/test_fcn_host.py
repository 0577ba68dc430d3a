"""FCNHead decode head and auxiliary head, host side (no GPU): construction, keys, initialisation, the weight
decay split, the refused criterion combinations, the new header's binding table and train.py's flags."""
import os
import sys

import pytest
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from rgbx_semantic_segmentation_amd.models.builder import PE1_KPAD, EncoderDecoder, backward_segment  # noqa: E402
from rgbx_semantic_segmentation_amd.models.decoders.fcnhead import FCNHead  # noqa: E402
from rgbx_semantic_segmentation_amd.params import ParamStore  # noqa: E402
from fcn_ref import FCNHeadRef, ref_model  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 9
HEAD_KEYS = {"conv.0.weight", "conv.0.bias", "conv.1.weight", "conv.1.bias", "conv.1.running_mean",
             "conv.1.running_var", "conv.1.num_batches_tracked", "classifier.weight", "classifier.bias"}


def test_fcn_decoder_builds():
    m = EncoderDecoder(dict(decoder="FCNHead", backbone="mit_b0", num_classes=K))
    h = m.decode_head
    assert isinstance(h, FCNHead) and h.out_index == 3 and m.aux_head is None
    assert (h.in_channels, h.channels, h.kernel_size, h.dropout_ratio) == (256, 64, 3, 0)
    assert set(h.state_dict()) == HEAD_KEYS
    assert h.conv[0].weight.shape == (64, 256, 3, 3) and h.classifier.weight.shape == (K, 64, 1, 1)


def test_aux_head_builds_beside_every_decoder():
    for decoder in ("MLPDecoder", "MLPDecoderpp", "FCNHead"):
        m = EncoderDecoder(dict(decoder=decoder, backbone="mit_b0", num_classes=K, aux_head=True))
        assert isinstance(m.aux_head, FCNHead) and m.aux_index == 2 and m.aux_rate == 0.4
        assert m.aux_head.in_channels == m.channels[2] == 160 and m.aux_head.channels == 40
        assert m.aux_head.out_index == 2 and set(m.aux_head.state_dict()) == HEAD_KEYS
    assert EncoderDecoder(dict(backbone="mit_b0", aux_head=True, aux_rate=0.25)).aux_rate == 0.25
    assert EncoderDecoder(dict(backbone="mit_b0")).aux_head is None


@pytest.mark.parametrize("cin", [160, 256, 320, 512, 384, 768])
def test_constructor_and_keys_are_the_references(cin):
    """The restatement (the reference's registration names) loads strictly into the product head and back."""
    torch.manual_seed(0)
    ref = FCNHeadRef(cin, num_classes=K)
    head = FCNHead(cin, num_classes=K)
    assert head.channels == cin // 4
    assert set(head.state_dict()) == HEAD_KEYS == set(ref.state_dict())
    head.load_state_dict(ref.state_dict(), strict=True)
    assert FCNHead(384, 32, 1, 1, 7).conv[0].weight.shape == (32, 384, 1, 1)       # positional order of the reference


def test_refused_constructions():
    with pytest.raises(NotImplementedError, match="dilation"):
        FCNHead(256, dilation=2)
    with pytest.raises(NotImplementedError, match="kernel_size"):
        FCNHead(256, kernel_size=5)


def test_model_keys_equal_the_reference_models():
    torch.manual_seed(0)
    for fcn, aux, decoder in ((True, False, "FCNHead"), (False, True, "MLPDecoder"), (True, True, "FCNHead")):
        ref = ref_model("mit_b0", fcn_decoder=fcn, aux_head=aux, num_classes=K)
        m = EncoderDecoder(dict(decoder=decoder, backbone="mit_b0", num_classes=K, aux_head=aux,
                                decoder_embed_dim=512))
        assert set(m.state_dict()) == set(ref.state_dict())
        m.load_state_dict(ref.state_dict(), strict=True)


def test_init_weights_covers_both_heads():
    torch.manual_seed(0)
    m = EncoderDecoder(dict(decoder="FCNHead", backbone="mit_b2", num_classes=K, aux_head=True))
    for h in (m.decode_head, m.aux_head):
        conv, bn = h.conv[0], h.conv[1]
        fan_in = conv.weight.shape[1] * 9
        assert abs(conv.weight.std().item() / (2.0 / fan_in) ** 0.5 - 1) < 0.1
        assert bn.eps == 1e-3 and bn.momentum == 0.1
        assert bool((bn.weight == 1).all()) and bool((bn.bias == 0).all())


def test_weight_decay_split_and_segments():
    m = EncoderDecoder(dict(decoder="FCNHead", backbone="mit_b0", num_classes=K, aux_head=True))
    st = ParamStore(m, "cpu", torch.float32, conv_pad={"backbone.patch_embed1.proj.weight": PE1_KPAD,
                                                       "backbone.extra_patch_embed1.proj.weight": PE1_KPAD},
                    segment_of=backward_segment)
    seen = set()
    for n, s in st.slots.items():
        if not (n.startswith("decode_head.") or n.startswith("aux_head.")):
            continue
        seen.add(n)
        decay = n.endswith("conv.0.weight") or n.endswith("classifier.weight")
        assert s.decay == decay and not s.frozen and backward_segment(n) == 0, n
        if n.endswith("conv.0.weight"):
            assert s.kind == "conv_taps" and s.storage_shape[1:3] == (3, 3)
    assert len(seen) == 12


def _criteria():
    from rgbx_semantic_segmentation_amd.utils.loss_opr import DiceCELoss, DiceLoss, FocalLoss, ProbOhemCrossEntropy2d
    return {"DiceLoss": DiceLoss(ignore_index=255, reduction="mean"),
            "DiceCELoss": DiceCELoss(alpha=0.5, ignore_index=255, reduction="mean"),
            "ProbOhemCrossEntropy2d": ProbOhemCrossEntropy2d(255, reduction="mean", thresh=0.6, min_kept=16),
            "CE_Focal": (nn.CrossEntropyLoss(reduction="mean", ignore_index=255),
                         FocalLoss(ignore_label=255, gamma=4.0, alpha=0.25, reduction="mean"))}


@pytest.mark.parametrize("name", ["DiceLoss", "DiceCELoss", "ProbOhemCrossEntropy2d"])
@pytest.mark.parametrize("cfg", [dict(decoder="FCNHead"), dict(aux_head=True), dict(decoder="MLPDecoderpp",
                                                                                    aux_head=True)])
def test_refused_criteria(name, cfg):
    with pytest.raises(NotImplementedError, match=f"{name} with (decoder='FCNHead'|aux_head).*x4 only"):
        EncoderDecoder(dict(backbone="mit_b0", **cfg), criterion=_criteria()[name])
    EncoderDecoder(dict(backbone="mit_b0"), criterion=_criteria()[name])            # at x4 it stays supported


def test_ce_focal_main_head_only():
    crit = _criteria()["CE_Focal"]
    EncoderDecoder(dict(backbone="mit_b0", decoder="FCNHead"), criterion=crit)
    for cfg in (dict(aux_head=True), dict(decoder="FCNHead", aux_head=True)):
        with pytest.raises(NotImplementedError, match="CE_Focal with aux_head.*tuple"):
            EncoderDecoder(dict(backbone="mit_b0", **cfg), criterion=crit)


def test_header_table_and_abi():
    from rgbx_semantic_segmentation_amd import _lib
    sigs = _lib.parse_header(os.path.join(ROOT, "include", "cmx_fcn.h"))
    assert tuple(sigs) == ("cmx_upsample_loss_scaled_workspace", "cmx_upsample_loss_scaled_fwd_adj")
    assert tuple(sigs) == tuple(_lib.FCN_SIGNATURES)
    assert _lib.header_abi_version() == 7 and _lib.query("cmx_abi_version") == 7
    for name in sigs:
        assert _lib.FCN_SIGNATURES[name].kinds == sigs[name].kinds
        assert name not in _lib.SIGNATURES and getattr(_lib.LIB, name) is not None
    kinds = sigs["cmx_upsample_loss_scaled_fwd_adj"].kinds
    assert len(kinds) == 19 and kinds[:6] == (_lib.POINTER,) * 6 and kinds[-1] == _lib.STREAM
    assert set(kinds[6:-1]) == {_lib.SCALAR}
    # the size query launches nothing: 2 floats per workgroup (1024 / S^2 cells each) + 4 x 40 per cell
    for S, cpw in ((8, 16), (16, 4), (32, 1)):
        B, h, w = 2, 30, 40
        groups = (w + 1 + cpw - 1) // cpw
        want = 4 * (2 * B * (h + 1) * groups + B * (h + 1) * (w + 1) * 160)
        assert _lib.query("cmx_upsample_loss_scaled_workspace", B, h, w, S) == want
    assert _lib.query("cmx_upsample_loss_scaled_workspace", 2, 30, 40, 4) == 0
    assert _lib.query("cmx_upsample_loss_scaled_workspace", 0, 30, 40, 16) == 0


def test_train_parser_and_criterion_check():
    import train
    p = train.build_parser()
    a = p.parse_args([])
    assert a.decoder == "MLPDecoder" and a.aux_head is False and a.aux_rate == 0.4
    a = p.parse_args(["--decoder", "FCNHead", "--aux-head", "--aux-rate", "0.3"])
    assert a.decoder == "FCNHead" and a.aux_head is True and a.aux_rate == 0.3
    with pytest.raises(SystemExit):
        p.parse_args(["--decoder", "UPernet"])
    assert isinstance(train.build_criterion(a), nn.CrossEntropyLoss)
    for extra, what in ((["--criterion", "ProbOhemCrossEntropy2d"], "ProbOhemCrossEntropy2d"),
                        (["--dice-alpha", "0.5"], "DiceCELoss"), (["--criterion", "CE_Focal"], "CE_Focal")):
        with pytest.raises(NotImplementedError, match=what):
            train.build_criterion(p.parse_args(["--aux-head"] + extra))
    train.build_criterion(p.parse_args(["--decoder", "FCNHead", "--criterion", "CE_Focal"]))
    train.build_criterion(p.parse_args(["--criterion", "ProbOhemCrossEntropy2d"]))
