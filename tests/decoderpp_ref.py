"""Restatement of the MLPDecoderpp decode head (reference: models/decoders/MLPDecoderpp.py:22-89)
for parity tests, in the style of oracle/cmx_ref.py: plain torch modules that run in any dtype
(the tests use fp64 on the CPU), written from the head's formulas:

    fused = GELU(BN(conv1x1(cat(c1', up(c2'), up(c3'), up(c4')))))       :74-80   (c_i' = conv1x1(c_i))
    a     = sigmoid(W2 GELU(W1 avgpool_hw(fused) + b1) + b2)             :55-61, :81
    out   = Dropout2d(fused * a)                                          :82-85
    pred  = conv1x1(out)                                                  :88

state_dict keys as the reference's (:42-64): linear_c{1..4}.{weight,bias} (Conv2d), linear_fuse.0 /
linear_fuse.1, attention.1 / attention.3, linear_pred.  The Dropout2d takes an injectable (B, E)
keep mask, as oracle.cmx_ref.Dropout2d does.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle.cmx_ref import Dropout2d, decoder_init


class DecoderHeadPP(nn.Module):
    def __init__(self, in_channels, num_classes, embed_dim, dropout_ratio=0.1, bn_eps=1e-3, bn_momentum=0.1):
        super().__init__()
        E = embed_dim
        for i, c in enumerate(in_channels):
            setattr(self, f"linear_c{i + 1}", nn.Conv2d(c, E, 1))                        # :42-45
        self.linear_fuse = nn.Sequential(nn.Conv2d(4 * E, E, 1), nn.BatchNorm2d(E, eps=bn_eps, momentum=bn_momentum),
                                         nn.GELU())                                      # :48-52
        self.attention = nn.Sequential(nn.AdaptiveAvgPool2d(1), nn.Conv2d(E, E // 4, 1), nn.GELU(),
                                       nn.Conv2d(E // 4, E, 1), nn.Sigmoid())            # :55-61
        self.linear_pred = nn.Conv2d(E, num_classes, 1)                                  # :64
        self.dropout = Dropout2d(dropout_ratio)                                          # :66
        decoder_init(self, bn_eps, bn_momentum)

    def forward(self, inputs):
        size = inputs[0].shape[2:]
        branches = []
        for i, c in enumerate(inputs):                                                   # :74-77
            t = getattr(self, f"linear_c{i + 1}")(c)
            branches.append(t if i == 0 else F.interpolate(t, size=size, mode="bilinear", align_corners=False))
        fused = self.linear_fuse(torch.cat(branches, 1))                                 # :80, c1 first
        fused = fused * self.attention(fused)                                            # :81-82
        return self.linear_pred(self.dropout(fused))                                     # :84-88


def gate(y, W1, b1, W2, b2, dscale=None):
    """The gate on token-major y (B, N, C): (pooled, hidden pre-activation, a, out), in y's dtype."""
    pooled = y.mean(1)
    z1 = pooled @ W1.t() + b1
    a = torch.sigmoid(F.gelu(z1) @ W2.t() + b2)
    f = a if dscale is None else a * dscale
    return pooled, z1, a, y * f[:, None, :]
