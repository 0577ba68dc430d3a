"""The UPerNet decode head (models/decoders/UPernet.py:8-146 of the reference, ``UPerHead`` with its ``PPM``) restated
in plain PyTorch for the tests: the reference's registration names (``psp_modules.{0..3}.{1,2}``, ``bottleneck.{0,1}``,
``lateral_convs.{0..2}.{0,1}``, ``fpn_convs.{0..2}.{0,1}``, ``fpn_bottleneck.{0,1}``, ``conv_seg``), any floating dtype
including fp64, and the top-down pass as an OUT-OF-PLACE sum: the reference's ``laterals[i - 1] += up(laterals[i])``
overwrites a ReLU output that autograd saved, so its own backward raises; the forward values are the same
(tests/test_uper_host.py ties them to outputs recorded from the reference's own class, tests/golden/uperhead_fwd.npz).
``ref_model`` is oracle.cmx_ref.EncoderDecoder carrying this head and, by default as in the reference
(builder.py:163-170), the restated auxiliary FCNHead of tests/fcn_ref.py.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from easpp_ref import jitter, settle_kinks  # noqa: F401  (re-exported)
from fcn_ref import FCNRefModel
from oracle.cmx_ref import CMXConfig, decoder_init

POOL_SCALES = (1, 2, 3, 6)


def _unit(cin, cout, k):
    return nn.Sequential(nn.Conv2d(cin, cout, k, padding=k // 2), nn.BatchNorm2d(cout), nn.ReLU())


def _up(t, size):
    return F.interpolate(t, size=size, mode="bilinear", align_corners=False)


class UPerHeadRef(nn.Module):
    def __init__(self, in_channels, num_classes=40, channels=512, pool_scales=POOL_SCALES):
        super().__init__()
        c4 = in_channels[-1]
        self.psp_modules = nn.ModuleList(nn.Sequential(nn.AdaptiveAvgPool2d(s), *_unit(c4, channels, 1))
                                         for s in pool_scales)
        self.bottleneck = _unit(c4 + len(pool_scales) * channels, channels, 3)
        self.lateral_convs = nn.ModuleList(_unit(c, channels, 1) for c in in_channels[:-1])
        self.fpn_convs = nn.ModuleList(_unit(channels, channels, 3) for _ in in_channels[:-1])
        self.fpn_bottleneck = _unit(len(in_channels) * channels, channels, 3)
        self.conv_seg = nn.Conv2d(channels, num_classes, 1)
        # no Dropout2d in this head; the attribute takes the mask test_config_parity._masks hands every decode head
        self.dropout = nn.Identity()

    def forward(self, feats):
        x = feats[-1]
        psp = torch.cat([x] + [_up(m(x), x.shape[2:]) for m in self.psp_modules], 1)
        lat = [m(f) for m, f in zip(self.lateral_convs, feats)] + [self.bottleneck(psp)]
        for i in range(len(lat) - 1, 0, -1):
            lat[i - 1] = lat[i - 1] + _up(lat[i], lat[i - 1].shape[2:])
        outs = [m(t) for m, t in zip(self.fpn_convs, lat)] + [lat[-1]]
        size = outs[0].shape[2:]
        cat = torch.cat([outs[0]] + [_up(t, size) for t in outs[1:]], 1)
        return self.conv_seg(self.fpn_bottleneck(cat))


def ref_model(backbone="mit_b0", aux_head=True, criterion=None, **cfg):
    """fp32; the caller seeds torch first."""
    c = CMXConfig(backbone=backbone, **cfg)
    ref = FCNRefModel(c, False, aux_head, criterion=criterion)
    ref.decode_head = UPerHeadRef(ref.channels, c.num_classes)
    decoder_init(ref.decode_head, c.bn_eps, c.bn_momentum)
    return ref
