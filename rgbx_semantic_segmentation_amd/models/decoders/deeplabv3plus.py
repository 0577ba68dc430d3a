"""DeepLabV3+ decode head (reference: models/decoders/deeplabv3plus.py:6-98): ASPP on the stage-4 map, a 48-channel
3x3 projection of the stage-1 map, the ASPP output upsampled (bilinear, align_corners=True) onto the stage-1 grid and
concatenated with it, a 3x3 conv block and the classifier.  The logits live on the stage-1 grid (1/4 resolution), so
every x4 loss of the package applies.  Constructor and registration names are the reference's (``aspp.b0.{0,1}``,
``aspp.b{1,2,3}.block.{0,1}``, ``aspp.b4.gap.{1,2}``, ``aspp.project.{0,1}``, ``low_level.{0,1}``, ``block.{0,1,4}``),
so its checkpoints load strictly.

``run`` on token-major NHWC rows, in launches (forward):
  ASPP     b0 as a GEMM; b1..b3 (dilated 3x3, C4 -> 256, one shared input) as ONE grouped launch
           (functions.AsppConv3F, csrc/aspp_conv.hip); b4 = pool + tiny linear (functions.pooled_conv); five
           BatchNorm + ReLU; one launch assembles the 1280-wide concat with the pooled row broadcast
           (functions.EasppConcatF: bilinear align_corners=True of a 1x1 map is a broadcast); the projection GEMM; its
           BatchNorm + ReLU with the elementwise Dropout(0.5) as the scale of the same launch.
  decoder  low_level through functions.conv + BatchNorm + ReLU; ONE launch upsamples the ASPP output with the
           align_corners=True rule and writes the 304-wide concat (functions.UpcatAcF, csrc/upcat.hip); block[0]
           through functions.conv (Cin = 304 is no multiple of 64: im2col + GEMM); BatchNorm + ReLU with Dropout(0.1)
           as its scale; the classifier GEMM.
The two elementwise Dropouts draw their masks on the device, each from a step counter of its own, so a replayed HIP
graph draws fresh masks; the counters are made by the first training forward, which must be an eager one.
``forced_masks`` (set by the builder from the model's): ``"dlv3_aspp_dropout"`` (B, h4, w4, 256) and
``"dlv3_block_dropout"`` (B, h1, w1, 256), 0/1, for tests.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from ... import functions as F


class ASPPConv(nn.Module):                        # deeplabv3plus.py:37-47
    def __init__(self, in_channels, out_channels, atrous_rate, norm_layer):
        super().__init__()
        self.block = nn.Sequential(nn.Conv2d(in_channels, out_channels, 3, padding=atrous_rate, dilation=atrous_rate,
                                             bias=False), norm_layer(out_channels), nn.ReLU(True))


class AsppPooling(nn.Module):                     # deeplabv3plus.py:50-64
    def __init__(self, in_channels, out_channels, norm_layer):
        super().__init__()
        self.gap = nn.Sequential(nn.AdaptiveAvgPool2d(1), nn.Conv2d(in_channels, out_channels, 1, bias=False),
                                 norm_layer(out_channels), nn.ReLU(True))


class ASPP(nn.Module):                            # deeplabv3plus.py:67-98
    def __init__(self, in_channels, atrous_rates, norm_layer):
        super().__init__()
        out_channels = 256
        self.b0 = nn.Sequential(nn.Conv2d(in_channels, out_channels, 1, bias=False), norm_layer(out_channels),
                                nn.ReLU(True))
        rate1, rate2, rate3 = tuple(atrous_rates)
        self.b1 = ASPPConv(in_channels, out_channels, rate1, norm_layer)
        self.b2 = ASPPConv(in_channels, out_channels, rate2, norm_layer)
        self.b3 = ASPPConv(in_channels, out_channels, rate3, norm_layer)
        self.b4 = AsppPooling(in_channels, out_channels, norm_layer=norm_layer)
        self.project = nn.Sequential(nn.Conv2d(5 * out_channels, out_channels, 1, bias=False),
                                     norm_layer(out_channels), nn.ReLU(True), nn.Dropout(0.5))


class DeepLabV3Plus(nn.Module):
    def __init__(self, in_channels=[256, 512, 1024, 2048], num_classes=40, norm_layer=nn.BatchNorm2d):
        super().__init__()
        self.num_classes = num_classes
        self.in_channels = list(in_channels)
        self.dropout_ratio = 0          # EncoderDecoder._stochastic draws no Dropout2d mask for this head
        self.embed_dim = 256
        self.forced_masks = None
        self.aspp = ASPP(in_channels=in_channels[3], atrous_rates=[12, 24, 36], norm_layer=norm_layer)
        self.low_level = nn.Sequential(nn.Conv2d(in_channels[0], 48, kernel_size=3, stride=1, padding=1),
                                       norm_layer(48), nn.ReLU(inplace=True))
        self.block = nn.Sequential(nn.Conv2d(304, 256, kernel_size=3, stride=1, padding=1), norm_layer(256),
                                   nn.ReLU(inplace=True), nn.Dropout(0.1), nn.Conv2d(256, num_classes, 1))

    def dropout_scale(self, which, p, n, device):
        """An elementwise Dropout(p) as F.batchnorm's dscale (n values): forced_masks[which] if given, else drawn on
        the device from a seed and a device-side step counter of this dropout's own (eASPP.dropout_scale's scheme)."""
        if p <= 0:
            return None
        mask = self.forced_masks.get(which) if self.forced_masks is not None else None
        if mask is not None:
            return (mask.to(device=device, dtype=torch.float32).reshape(-1) / (1 - p)).contiguous()
        device = torch.device(device)
        states = self.__dict__.setdefault("_mask_states", {})
        st = states.get(which)
        if st is None or st[1].device.type != device.type or device.index not in (None, st[1].device.index):
            if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
                # made inside a capture the counter would live in the graph's pool, and its zero fill would be
                # replayed: every replay would draw the first mask again
                raise RuntimeError("DeepLabV3Plus: the dropout masks' device step counters must exist before a graph "
                                   "capture: run one eager training step first")
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())       # from torch's host generator
            st = states[which] = (seed, torch.zeros(2, dtype=torch.int64, device=device))
        return F.easpp_dropout_scale(st, n, p, device)

    def run(self, store, feats, grids, B, training, dscale=None, group=None):
        """feats: the four stage maps as (B * h_i * w_i, C_i) token rows, grids their (h_i, w_i).  Returns logits
        (B * h1 * w1, K) on the stage-1 grid."""
        (h1, w1), (h4, w4) = grids[0], grids[3]
        C1, C4 = self.in_channels[0], self.in_channels[3]
        M1, M4, N4 = B * h1 * w1, B * h4 * w4, h4 * w4
        if training and B == 1:
            raise ValueError("DeepLabV3Plus: training needs more than 1 image per batch: the pooled branch's "
                             "BatchNorm sees one value per channel (as torch.nn.BatchNorm2d refuses)")
        a = self.aspp

        def unit(bn, t, **kw):
            return F.batchnorm(store, bn, t, training, act="relu", group=group, **kw)

        # ---- ASPP on the stage-4 map
        x4 = feats[3].reshape(M4, C4)
        outs = [unit(a.b0[1], F.glinear(store, a.b0[0].weight, None, x4.view(1, M4, C4)).view(M4, -1))]
        branches = (a.b1, a.b2, a.b3)
        ys = F.aspp_conv3(store, [b.block[0] for b in branches], x4, B, h4, w4)
        outs += [unit(b.block[1], y) for b, y in zip(branches, ys)]
        gap = a.b4.gap
        pool = unit(gap[2], F.pooled_conv(store, gap[1], x4, B, N4))
        cat = F.EasppConcatF.apply(*outs, pool, B, N4)
        y = F.glinear(store, a.project[0].weight, None, cat.view(1, M4, -1)).view(M4, -1)
        scale = self.dropout_scale("dlv3_aspp_dropout", a.project[3].p, y.numel(), y.device) if training else None
        c4 = unit(a.project[1], y, dscale=scale, rps=1)
        # ---- decoder on the stage-1 grid
        low = self.low_level[0]
        x1 = feats[0].reshape(B, h1, w1, C1)
        c1, _, _ = F.conv(store, low, x1, 1, B, h1, w1, C1, 1, 1)
        c1 = unit(self.low_level[1], c1.view(M1, -1))
        cat = F.UpcatAcF.apply(c4, c1, (B, h4, w4, h1, w1))
        Cc = cat.shape[-1]
        z, _, _ = F.conv(store, self.block[0], cat.view(B, h1, w1, Cc), 1, B, h1, w1, Cc, 1, 1)
        scale = self.dropout_scale("dlv3_block_dropout", self.block[3].p, M1 * 256, z.device) if training else None
        f = unit(self.block[1], z.view(M1, -1), dscale=scale, rps=1)
        cls = self.block[4]
        return F.glinear(store, cls.weight, cls.bias, f.view(1, M1, -1)).view(M1, -1)
