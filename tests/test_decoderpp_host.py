"""MLPDecoderpp on the host (no GPU): the builder accepts it and still refuses the other decoders,
the head's state_dict is the reference's (models/decoders/MLPDecoderpp.py:42-64), the weight-decay
grouping is group_weight's rule for Conv2d, and the gate's entry points are pure additions to the
C-ABI (revision unchanged)."""
import pytest
import torch

from rgbx_semantic_segmentation_amd.models.builder import EncoderDecoder, PE1_KPAD, backward_segment
from rgbx_semantic_segmentation_amd.params import ParamStore

E, K = 256, 7
CH = (32, 64, 160, 256)          # mit_b0


def _model():
    torch.manual_seed(0)
    return EncoderDecoder(dict(decoder="MLPDecoderpp", backbone="mit_b0", num_classes=K, decoder_embed_dim=E))


def test_builder_constructs_mlpdecoderpp():
    m = _model()
    h = m.decode_head
    assert type(h).__module__.endswith("decoders.MLPDecoderpp")
    assert (h.dropout_ratio, h.embed_dim, h.in_channels, h.num_classes) == (0.1, E, list(CH), K)
    assert m.cmx_capturable


def test_state_dict_keys_and_shapes():
    sd = _model().decode_head.state_dict()
    want = {}
    for i, c in enumerate(CH):
        want[f"linear_c{i + 1}.weight"] = (E, c, 1, 1)
        want[f"linear_c{i + 1}.bias"] = (E,)
    want.update({"linear_fuse.0.weight": (E, 4 * E, 1, 1), "linear_fuse.0.bias": (E,),
                 "linear_fuse.1.weight": (E,), "linear_fuse.1.bias": (E,), "linear_fuse.1.running_mean": (E,),
                 "linear_fuse.1.running_var": (E,), "linear_fuse.1.num_batches_tracked": (),
                 "attention.1.weight": (E // 4, E, 1, 1), "attention.1.bias": (E // 4,),
                 "attention.3.weight": (E, E // 4, 1, 1), "attention.3.bias": (E,),
                 "linear_pred.weight": (K, E, 1, 1), "linear_pred.bias": (K,)})
    assert {k: tuple(v.shape) for k, v in sd.items()} == want


def test_state_dict_loads_from_the_restated_head():
    from decoderpp_ref import DecoderHeadPP
    ref = DecoderHeadPP(CH, K, E)
    _model().decode_head.load_state_dict(ref.state_dict(), strict=True)


def test_decoder_init_is_kaiming_on_every_conv():
    """init_weight walks decode_head.modules(): the attention convs too (fan_in, relu gain)."""
    h = _model().decode_head
    for conv in (h.attention[1], h.attention[3], h.linear_c1):
        fan_in = conv.weight.shape[1]
        assert abs(conv.weight.std().item() / (2.0 / fan_in) ** 0.5 - 1) < 0.1
    bn = h.linear_fuse[1]
    assert bn.eps == 1e-3 and bool((bn.weight == 1).all()) and bool((bn.bias == 0).all())


@pytest.mark.parametrize("decoder", ["UPernet", "deeplabv3+", "nearest"])
def test_other_decoders_still_refused(decoder):
    with pytest.raises(NotImplementedError) as e:
        EncoderDecoder(dict(decoder=decoder, backbone="mit_b0"))
    assert "MLPDecoder" in str(e.value) and "MLPDecoderpp" in str(e.value)


def test_default_decoder_unchanged():
    m = EncoderDecoder(dict(backbone="mit_b0", num_classes=K))
    assert type(m.decode_head).__module__.endswith("decoders.MLPDecoder")
    assert "linear_c1.proj.weight" in m.decode_head.state_dict()


def test_weight_decay_split():
    """attention.{1,3}.weight, linear_c*.weight, linear_fuse.0.weight and linear_pred.weight decay; every
    bias and the BN affine parameters do not; nothing in the head is frozen; the per-64-element
    flags of the flat buffer (what FusedAdamW / FusedSGD read) say the same."""
    m = _model()
    st = ParamStore(m, "cpu", torch.float32, conv_pad={"backbone.patch_embed1.proj.weight": PE1_KPAD,
                                                       "backbone.extra_patch_embed1.proj.weight": PE1_KPAD},
                    segment_of=backward_segment)
    decay = {"attention.1.weight", "attention.3.weight", "linear_c1.weight", "linear_c2.weight", "linear_c3.weight",
             "linear_c4.weight", "linear_fuse.0.weight", "linear_pred.weight"}
    seen = set()
    for n, s in st.slots.items():
        if not n.startswith("decode_head."):
            continue
        short = n[len("decode_head."):]
        seen.add(short)
        assert s.decay == (short in decay) and not s.frozen, n
        assert backward_segment(n) == 0
        flags = st.decay64[s.offset // 64:(s.offset + s.stride * s.count + 63) // 64]
        assert bool((flags == (1 if short in decay else 0)).all()), n
    assert decay <= seen and {"attention.1.bias", "attention.3.bias", "linear_fuse.1.weight"} <= seen


def test_abi_unchanged_and_symbols_resolve():
    from rgbx_semantic_segmentation_amd import _lib
    assert _lib.header_abi_version() == 7 and _lib.query("cmx_abi_version") == 7
    for name, nargs in (("cmx_se_pool_fwd", 9), ("cmx_se_scale_fwd", 9), ("cmx_se_bwd_reduce", 9),
                        ("cmx_se_bwd_apply", 12)):
        assert len(_lib.SIGNATURES[name][1]) == nargs
        assert getattr(_lib.LIB, name) is not None
    # the size queries launch nothing: chunks of at least cmx_se_chunk_rows() rows
    rows = _lib.query("cmx_se_chunk_rows")
    assert rows > 0
    assert _lib.query("cmx_se_pool_nchunk", 2, 1, 256) == 1
    assert _lib.query("cmx_se_pool_nchunk", 2, rows + 1, 256) == 2
    assert _lib.query("cmx_se_bwd_nslice", 2, 3 * rows, 256) == 3
    assert _lib.query("cmx_se_pool_workspace", 3, 2 * rows, 256) == 3 * 2 * 256 * 4
    assert _lib.query("cmx_se_pool_tickets", 3, 768) >= 3


def test_train_parser_has_decoder_switch():
    import train
    p = train.build_parser()
    assert p.parse_args([]).decoder == "MLPDecoder"
    assert p.parse_args(["--decoder", "MLPDecoderpp"]).decoder == "MLPDecoderpp"
    with pytest.raises(SystemExit):
        p.parse_args(["--decoder", "UPernet"])
