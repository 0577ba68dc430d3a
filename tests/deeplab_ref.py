"""The DeepLabV3+ decode head (models/decoders/deeplabv3plus.py:6-98 of the reference) restated in plain PyTorch for the
tests: the reference's registration names (``aspp.b0.{0,1}``, ``aspp.b{1,2,3}.block.{0,1}``, ``aspp.b4.gap.{1,2}``,
``aspp.project.{0,1}``, ``low_level.{0,1}``, ``block.{0,1,4}``), any floating dtype including fp64, and the two
elementwise Dropouts with keep masks that can be set (easpp_ref.MaskedDropout).  ``ref_model`` is
oracle.cmx_ref.EncoderDecoder carrying this head and, by default as in the reference (builder.py:172-179), the
restated auxiliary FCNHead of tests/fcn_ref.py.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from easpp_ref import MaskedDropout, jitter, settle_kinks  # noqa: F401  (jitter / settle_kinks: re-exported)
from fcn_ref import FCNRefModel
from oracle.cmx_ref import CMXConfig, decoder_init

RATES = (12, 24, 36)
WIDTH, LOW, P_ASPP, P_BLOCK = 256, 48, 0.5, 0.1


def _unit(cin, cout, k=1, rate=1):
    return nn.Sequential(nn.Conv2d(cin, cout, k, padding=rate * (k // 2), dilation=rate, bias=False),
                         nn.BatchNorm2d(cout), nn.ReLU())


class _Branch(nn.Module):                 # "block": the reference's ASPPConv registration name
    def __init__(self, cin, rate):
        super().__init__()
        self.block = _unit(cin, WIDTH, 3, rate)

    def forward(self, x):
        return self.block(x)


class _Pooled(nn.Module):                 # "gap": AsppPooling's
    def __init__(self, cin):
        super().__init__()
        self.gap = nn.Sequential(nn.AdaptiveAvgPool2d(1), *_unit(cin, WIDTH))

    def forward(self, x):
        # bilinear, align_corners=True, from a 1 x 1 map: every output pixel is that one value
        return self.gap(x).expand(-1, -1, *x.shape[2:])


class ASPPRef(nn.Module):
    def __init__(self, cin, rates=RATES):
        super().__init__()
        self.b0 = _unit(cin, WIDTH)
        self.b1, self.b2, self.b3 = (_Branch(cin, r) for r in rates)
        self.b4 = _Pooled(cin)
        self.project = nn.Sequential(*_unit(5 * WIDTH, WIDTH), MaskedDropout(P_ASPP))

    def forward(self, x):
        return self.project(torch.cat([b(x) for b in (self.b0, self.b1, self.b2, self.b3, self.b4)], 1))


class DeepLabV3PlusRef(nn.Module):
    def __init__(self, in_channels, num_classes=40):
        super().__init__()
        self.aspp = ASPPRef(in_channels[3])
        self.low_level = nn.Sequential(nn.Conv2d(in_channels[0], LOW, 3, padding=1), nn.BatchNorm2d(LOW), nn.ReLU())
        self.block = nn.Sequential(nn.Conv2d(WIDTH + LOW, WIDTH, 3, padding=1), nn.BatchNorm2d(WIDTH), nn.ReLU(),
                                   MaskedDropout(P_BLOCK), nn.Conv2d(WIDTH, num_classes, 1))
        # no Dropout2d in this head; the attribute takes the mask test_config_parity._masks hands every decode head
        self.dropout = nn.Identity()

    def set_masks(self, aspp_mask, block_mask):
        """NCHW keep masks of the two Dropouts (None: drawn)."""
        self.aspp.project[3].mask, self.block[3].mask = aspp_mask, block_mask

    def forward(self, feats):
        c1 = self.low_level(feats[0])
        c4 = F.interpolate(self.aspp(feats[3]), size=c1.shape[2:], mode="bilinear", align_corners=True)
        return self.block(torch.cat([c4, c1], 1))


def ref_model(backbone="mit_b0", aux_head=True, criterion=None, **cfg):
    """fp32; the caller seeds torch first."""
    c = CMXConfig(backbone=backbone, **cfg)
    ref = FCNRefModel(c, False, aux_head, criterion=criterion)
    ref.decode_head = DeepLabV3PlusRef(ref.channels, c.num_classes)
    decoder_init(ref.decode_head, c.bn_eps, c.bn_momentum)
    return ref
