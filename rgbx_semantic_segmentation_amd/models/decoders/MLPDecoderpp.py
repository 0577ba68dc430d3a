"""MLPDecoderpp decode head (reference: models/decoders/MLPDecoderpp.py:22-89): the all-MLP head
with 1x1-conv projections, a GELU after the fuse BatchNorm and a channel-attention
(squeeze-excite) gate on the fused map.

Execution on tokens: linear_c{1..4} (1x1 convs: the products of MLPDecoder's Linears), the
upsample, the concat [c1 | c2 | c3 | c4] (:80, c1 FIRST, the reverse of MLPDecoder's) and the
linear_fuse 1x1 conv as functions.DecoderFoldC1F (CMX_DECODER_FOLD=0: one multi GEMM launch ahead
of functions.DecoderFuseC1F); BatchNorm (SyncBN across ranks when a process group is given) + GELU
in one apply kernel; the gate and the Dropout2d as functions.SEGateF (se_gate.hip); linear_pred
GEMM.  Returns low-resolution logits (B*N1, K).
"""
from __future__ import annotations

import torch.nn as nn

from ... import functions as F


class DecoderHead(nn.Module):
    def __init__(self, in_channels=(64, 128, 320, 512), num_classes=40, dropout_ratio=0.1,
                 norm_layer=nn.BatchNorm2d, embed_dim=512, align_corners=False):
        super().__init__()
        if align_corners:
            raise NotImplementedError("MLPDecoderpp: align_corners=True is not on the CMX hot path")
        if embed_dim % 16:
            raise ValueError(f"MLPDecoderpp: embed_dim {embed_dim} must be a multiple of 16 (the gate's hidden "
                             "width embed_dim / 4 in 16-byte vectors)")
        self.num_classes = num_classes
        self.dropout_ratio = dropout_ratio
        self.align_corners = align_corners
        self.in_channels = list(in_channels)
        self.embed_dim = embed_dim
        c1, c2, c3, c4 = in_channels
        self.linear_c1 = nn.Conv2d(c1, embed_dim, 1)
        self.linear_c2 = nn.Conv2d(c2, embed_dim, 1)
        self.linear_c3 = nn.Conv2d(c3, embed_dim, 1)
        self.linear_c4 = nn.Conv2d(c4, embed_dim, 1)
        self.linear_fuse = nn.Sequential(nn.Conv2d(4 * embed_dim, embed_dim, 1), nn.BatchNorm2d(embed_dim), nn.GELU())
        self.attention = nn.Sequential(nn.AdaptiveAvgPool2d(1), nn.Conv2d(embed_dim, embed_dim // 4, 1), nn.GELU(),
                                       nn.Conv2d(embed_dim // 4, embed_dim, 1), nn.Sigmoid())
        self.linear_pred = nn.Conv2d(embed_dim, num_classes, 1)

    def run(self, store, feats, grids, B, training, dscale=None, group=None):
        E = self.embed_dim
        lin = (self.linear_c1, self.linear_c2, self.linear_c3, self.linear_c4)
        H1, W1 = grids[0]
        N1 = H1 * W1
        M = B * N1
        conv = self.linear_fuse[0]
        G = 1
        Wf = store.w(conv.weight).view(G, E, 4 * E)
        Wfg = store.g(conv.weight).view(G, E, 4 * E)
        bf = store.w(conv.bias, compute=False).view(G, E)
        bfg = store.g(conv.bias).view(G, E)
        sizes = [grids[0]] + list(grids[1:])
        if F.DECODER_FOLD:
            # linear_c{1..4} folded into linear_fuse: M_i = Wf_i Wc_i formed per step (DecoderFoldC1F);
            # the (E, C_i, 1, 1) conv weights are stored (E, C_i), Wf's column slots are c1, c2, c3, c4
            Wc = tuple(store.w(m.weight, stacked=False) for m in lin)
            bc = tuple(store.w(m.bias, stacked=False, compute=False) for m in lin)
            grads = (Wfg, bfg.view(E), tuple(store.g(m.weight) for m in lin),
                     tuple(store.g(m.bias, stacked=False) for m in lin))
            x = [t.view(B, -1, t.shape[-1]) for t in feats]
            f = F.DecoderFoldC1F.apply(x[3], x[2], x[1], x[0], Wf[0], Wc, bf.view(E), bc, grads, sizes, conv.weight)
        else:
            # the four projections as ONE GEMM launch (and their input gradients as another)
            outs = F.glinear_multi(store, [(lin[i].weight, lin[i].bias, feats[i].view(1, -1, feats[i].shape[-1]))
                                           for i in range(4)])
            proj = [t.view(B, -1, E) for t in outs]
            f = F.DecoderFuseC1F.apply(proj[3], proj[2], proj[1], proj[0], Wf, Wfg, bf, bfg, sizes, conv.weight)
        f = F.batchnorm(store, self.linear_fuse[1], f.view(M, E), training, act="gelu", dscale=None, rps=N1,
                        group=group)
        f = F.se_gate(store, self.attention, f.view(B, N1, E), dscale=dscale)
        return F.glinear(store, self.linear_pred.weight, self.linear_pred.bias, f.view(1, M, E)).view(M, -1)
