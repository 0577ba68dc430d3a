"""FCNHead (models/decoders/fcnhead.py:9-29 of the reference) restated in plain PyTorch for the tests, with the
reference's registration names (``conv.0``, ``conv.1``, ``classifier``), in any floating dtype including fp64; and
``ref_model``: oracle.cmx_ref.EncoderDecoder carrying it as the FCN-32s decode head on the stage-4 map
(builder.py:186-189) and / or as the auxiliary head on the stage-3 map with the loss
``main + aux_rate * criterion(aux logits upsampled, label)`` (builder.py:167-170, 234-237, 250-251).
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle.cmx_ref import CMXConfig, EncoderDecoder, decoder_init


class FCNHeadRef(nn.Module):
    def __init__(self, in_channels, channels=None, kernel_size=3, num_classes=40):
        super().__init__()
        channels = channels or in_channels // 4
        self.conv = nn.Sequential(nn.Conv2d(in_channels, channels, kernel_size, padding=kernel_size // 2),
                                  nn.BatchNorm2d(channels), nn.ReLU())
        self.classifier = nn.Conv2d(channels, num_classes, 1)
        # no Dropout2d in this head; the attribute takes the mask test_config_parity._masks hands every decode head
        self.dropout = nn.Identity()

    def forward(self, x):
        return self.classifier(self.conv(x))


def jitter(head, g, dtype=torch.float32):
    """Non-trivial BN affine parameters and running statistics, then every parameter rounded to ``dtype`` (values
    both sides can store), as easpp_ref.jitter."""
    with torch.no_grad():
        for m in head.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.weight.add_(0.1 * torch.randn(m.weight.shape, generator=g))
                m.bias.add_(0.1 * torch.randn(m.bias.shape, generator=g))
                m.running_mean.copy_(torch.rand(m.running_mean.shape, generator=g) * 0.2 - 0.1)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)
        for p in head.parameters():
            p.copy_(p.to(dtype))
    return head


class FCNRefModel(EncoderDecoder):
    """The oracle with decode_head and / or aux_head replaced by the restated FCN head."""

    def __init__(self, cfg, fcn_decoder, aux_head, aux_rate=0.4, criterion=None):
        super().__init__(cfg, criterion)
        if fcn_decoder:
            self.decode_head = FCNHeadRef(self.channels[-1], num_classes=cfg.num_classes)
            decoder_init(self.decode_head, cfg.bn_eps, cfg.bn_momentum)
        self.fcn_decoder = fcn_decoder
        self.aux_index, self.aux_rate = 2, aux_rate
        if aux_head:
            self.aux_head = FCNHeadRef(self.channels[2], num_classes=cfg.num_classes)
            decoder_init(self.aux_head, cfg.bn_eps, cfg.bn_momentum)

    def _up(self, t, size):
        return F.interpolate(t, size=size, mode="bilinear", align_corners=False)

    def encode_decode(self, rgb, modal_x, with_aux=False):
        feats = self.backbone(rgb, modal_x)
        out = self._up(self.decode_head(feats[-1] if self.fcn_decoder else feats), rgb.shape[2:])
        if with_aux and self.aux_head is not None:
            return out, self._up(self.aux_head(feats[self.aux_index]), rgb.shape[2:])
        return out

    def forward(self, rgb, modal_x, label=None):
        if label is None:
            return self.encode_decode(rgb, modal_x)
        if self.aux_head is None:
            return self.criterion(self.encode_decode(rgb, modal_x), label.long())
        out, aux = self.encode_decode(rgb, modal_x, with_aux=True)
        return self.criterion(out, label.long()) + self.aux_rate * self.criterion(aux, label.long())


def ref_model(backbone="mit_b0", fcn_decoder=False, aux_head=False, criterion=None, **cfg):
    """fp32; the caller seeds torch first."""
    return FCNRefModel(CMXConfig(backbone=backbone, **cfg), fcn_decoder, aux_head, criterion=criterion)
