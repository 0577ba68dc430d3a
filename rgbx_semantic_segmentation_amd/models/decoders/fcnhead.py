"""FCN head (reference: models/decoders/fcnhead.py:9-29): conv k x k + BatchNorm + ReLU, then a 1x1 classifier,
on ONE stage map.  The reference uses it as the FCN-32s decode head on the stage-4 map (builder.py:186-189) and
as the auxiliary head on the stage-3 map (builder.py:167-170); its logits live on that stage's grid
(``out_index``), so the loss upsamples them by 32 or 16 (functions.UpsampleScaledLossF).

Execution on token-major NHWC rows: the conv through functions.conv with G = 1 (the implicit GEMM for 16-bit
and Cin % 64 == 0, else im2col + GEMM; the weight is stored tap-major by the ParamStore), BatchNorm (SyncBN
across ranks when a process group is given) + ReLU as one functions.batchnorm, the classifier a GEMM.
Constructor and state_dict keys are the reference's.  There is no Dropout2d in this head.
"""
from __future__ import annotations

import torch.nn as nn

from ... import functions as F


class FCNHead(nn.Module):
    def __init__(self, in_channels=384, channels=None, kernel_size=3, dilation=1, num_classes=40,
                 norm_layer=nn.BatchNorm2d):
        super().__init__()
        if dilation != 1:
            raise NotImplementedError(f"FCNHead(dilation={dilation!r}): only dilation 1 is on the CMX hot path")
        if kernel_size not in (1, 3):
            raise NotImplementedError(f"FCNHead(kernel_size={kernel_size!r}): only 1 and 3 are on the CMX hot path")
        self.kernel_size = kernel_size
        self.in_channels = in_channels
        self.channels = channels or in_channels // 4
        self.num_classes = num_classes
        self.dropout_ratio = 0          # EncoderDecoder._stochastic draws no Dropout2d mask for this head
        self.embed_dim = self.channels
        self.out_index = 3              # the stage whose grid the logits live on (the builder sets 2 for the aux head)
        conv_padding = (kernel_size // 2) * dilation
        self.conv = nn.Sequential(nn.Conv2d(self.in_channels, self.channels, kernel_size, padding=conv_padding),
                                  norm_layer(self.channels), nn.ReLU(inplace=True))
        self.classifier = nn.Conv2d(self.channels, num_classes, kernel_size=1)

    def run(self, store, x, B, h, w, training, group=None):
        """x: the stage map as (B * h * w, Cin) token rows.  Returns low-resolution logits (B * h * w, K)."""
        C, E, M = self.in_channels, self.channels, B * h * w
        conv = self.conv[0]
        if self.kernel_size == 1:
            y = F.glinear(store, conv.weight, conv.bias, x.view(1, M, C))
        else:
            y, _, _ = F.conv(store, conv, x.view(B, h, w, C), 1, B, h, w, C, 1, self.kernel_size // 2)
        f = F.batchnorm(store, self.conv[1], y.view(M, E), training, act="relu", rps=h * w, group=group)
        return F.glinear(store, self.classifier.weight, self.classifier.bias, f.view(1, M, E)).view(M, -1)
