"""UPerNet decode head (reference: models/decoders/UPernet.py:8-146, ``UPerHead`` and ``PPM``): pyramid pooling on the
stage-4 map, an FPN over the four stage maps with a top-down pass, the four FPN outputs upsampled (bilinear,
align_corners=False) onto the stage-1 grid and concatenated, a 3x3 bottleneck and the classifier.  The logits live on
the stage-1 grid (1/4 resolution), so every x4 loss of the package applies.  Constructor and registration names are the
reference's (``psp_modules.{0..3}.{1,2}``, ``bottleneck.{0,1}``, ``lateral_convs.{0..2}.{0,1}``,
``fpn_convs.{0..2}.{0,1}``, ``fpn_bottleneck.{0,1}``, ``conv_seg``), so its checkpoints load strictly.  Every conv has a
bias; the head has no dropout (the reference's ``dropout_ratio`` argument is accepted and, as there, unused).

The forward VALUES are the reference's.  Its top-down pass is written ``laterals[i - 1] += up(laterals[i])``, which
overwrites a ReLU output autograd saved, so the reference's own backward raises; the gradient here is that of the
out-of-place form ``laterals[i - 1] = laterals[i - 1] + up(...)``: the ReLU mask of lateral i - 1 comes from its own
pre-sum value (functions.UpAddF writes a new tensor).  Training with one image per batch raises ValueError, as
torch.nn.BatchNorm2d does for the scale-1 pooling branch.

``run`` on token-major NHWC rows, in launches (forward):
  PPM        ONE launch pools the stage-4 map at the four scales (functions.PpmPoolF, csrc/uper.hip); per scale a GEMM
             C4 -> channels with bias on its block of pooled rows (functions.glinear) and BatchNorm + ReLU
             (functions.batchnorm); ONE launch upsamples the four results and writes the (C4 + 4 channels)-wide concat
             behind the stage-4 map (functions.UpcatMultiF); ``bottleneck`` through functions.conv + BatchNorm + ReLU.
  laterals   three GEMMs C_i -> channels + BatchNorm + ReLU.
  top-down   three launches ``hi + up(lo)`` (functions.UpAddF), each on the already updated level above.
  FPN        three 3x3 convs + BatchNorm + ReLU; ONE launch upsamples levels 1..3 onto the stage-1 grid and writes the
             4 channels-wide concat behind level 0 (functions.UpcatMultiF); ``fpn_bottleneck`` through functions.conv +
             BatchNorm + ReLU; the classifier GEMM.
The five 3x3 convs ask functions.conv for the im2col-free input gradient (``dgrad_implicit``): at mit_b2 480 x 640
bs = 2 the dcols buffer of ``fpn_bottleneck`` alone would be 1.42 GB.  fp32 compute stays on im2col + GEMM both ways (a
test vehicle at small shapes).
"""
from __future__ import annotations

import torch.nn as nn

from ... import functions as F


class PPM(nn.ModuleList):                         # UPernet.py:107-146
    def __init__(self, pool_scales, in_channel, channels, norm_layer, align_corners=False):
        super().__init__()
        self.pool_scales = tuple(pool_scales)
        self.align_corners = align_corners
        self.in_channel = in_channel
        self.channels = channels
        for s in self.pool_scales:
            self.append(nn.Sequential(nn.AdaptiveAvgPool2d(s), nn.Conv2d(in_channel, channels, 1),
                                      norm_layer(channels), nn.ReLU(inplace=True)))


class UPerHead(nn.Module):
    def __init__(self, in_channels=[96, 192, 384, 768], num_classes=40, channels=512, pool_scales=(1, 2, 3, 6),
                 norm_layer=nn.BatchNorm2d, dropout_ratio=0.1, align_corners=False):
        super().__init__()
        pool_scales = tuple(pool_scales)
        if len(pool_scales) != 4 or any(int(s) != s or not 1 <= s <= 8 for s in pool_scales):
            raise NotImplementedError(f"UPerHead(pool_scales={pool_scales!r}): four scales in 1..8 are on the CMX hot "
                                      "path (one pooling launch, cmx_ppm_pool_fwd)")
        if align_corners:
            raise NotImplementedError("UPerHead(align_corners=True): the head's upsample kernels follow the "
                                      "align_corners=False rule, the reference's default")
        if len(in_channels) != 4:
            raise NotImplementedError(f"UPerHead(in_channels={in_channels!r}): four stage maps")
        self.in_channels = list(in_channels)
        self.num_classes = num_classes
        self.channels = channels
        self.pool_scales = tuple(int(s) for s in pool_scales)
        self.align_corners = False
        self.dropout_ratio = 0          # EncoderDecoder._stochastic draws no Dropout2d mask for this head
        self.embed_dim = channels
        Ch = channels

        def unit(cin, k):
            return nn.Sequential(nn.Conv2d(cin, Ch, k, padding=k // 2), norm_layer(Ch), nn.ReLU())

        self.psp_modules = PPM(self.pool_scales, self.in_channels[-1], Ch, norm_layer=norm_layer, align_corners=False)
        self.bottleneck = unit(self.in_channels[-1] + len(self.pool_scales) * Ch, 3)
        self.lateral_convs = nn.ModuleList(unit(c, 1) for c in self.in_channels[:-1])
        self.fpn_convs = nn.ModuleList(unit(Ch, 3) for _ in self.in_channels[:-1])
        self.fpn_bottleneck = unit(len(self.in_channels) * Ch, 3)
        self.conv_seg = nn.Conv2d(Ch, num_classes, kernel_size=1)

    def run(self, store, feats, grids, B, training, dscale=None, group=None):
        """feats: the four stage maps as (B * h_i * w_i, C_i) token rows, grids their (h_i, w_i).  Returns logits
        (B * h1 * w1, K) on the stage-1 grid.  dscale (the Dropout2d scale of other heads) is unused: no dropout."""
        if training and B == 1:
            raise ValueError("UPerHead: training needs more than 1 image per batch: the scale-1 pooling branch's "
                             "BatchNorm sees one value per channel (as torch.nn.BatchNorm2d refuses)")
        Ch, Cin, scales = self.channels, self.in_channels, self.pool_scales
        Ms = [B * h * w for h, w in grids]

        def unit(bn, t):
            return F.batchnorm(store, bn, t, training, act="relu", group=group)

        def conv3(seq, t, i):
            h, w = grids[i]
            C = t.shape[-1]
            y, _, _ = F.conv(store, seq[0], t.view(B, h, w, C), 1, B, h, w, C, 1, 1, dgrad_implicit=True)
            return unit(seq[1], y.view(Ms[i], Ch))

        # ---- PPM on the stage-4 map: its gradient from the concat's skip columns goes through the pooling backward
        (h4, w4), C4 = grids[3], Cin[3]
        x4 = feats[3].reshape(Ms[3], C4)
        tap = F.ColumnTap()
        srcs = []
        for seq, blk in zip(self.psp_modules, F.PpmPoolF.apply(x4, (B, h4, w4, scales), tap)):
            n = blk.shape[0]
            srcs.append(unit(seq[2], F.glinear(store, seq[1].weight, seq[1].bias, blk.view(1, n, C4)).view(n, Ch)))
        cat = F.UpcatMultiF.apply((B, h4, w4, tuple((s, s) for s in scales)), tap, x4, *srcs)
        laterals = [None, None, None, conv3(self.bottleneck, cat, 3)]
        # ---- laterals and the top-down pass (each step on the already updated level above)
        for i, seq in enumerate(self.lateral_convs):
            y = F.glinear(store, seq[0].weight, seq[0].bias, feats[i].reshape(1, Ms[i], Cin[i])).view(Ms[i], Ch)
            laterals[i] = unit(seq[1], y)
        for i in (3, 2, 1):
            laterals[i - 1] = F.UpAddF.apply(laterals[i - 1], laterals[i], (B, *grids[i], *grids[i - 1]))
        # ---- FPN outputs, their concat on the stage-1 grid, the bottleneck and the classifier
        outs = [conv3(seq, laterals[i], i) for i, seq in enumerate(self.fpn_convs)] + [laterals[3]]
        cat = F.UpcatMultiF.apply((B, *grids[0], tuple(grids[1:])), None, *outs)
        f = conv3(self.fpn_bottleneck, cat, 0)
        cls = self.conv_seg
        return F.glinear(store, cls.weight, cls.bias, f.view(1, Ms[0], Ch)).view(Ms[0], -1)
