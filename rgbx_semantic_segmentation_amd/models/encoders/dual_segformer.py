"""Dual-stream MiT encoder (mit_b0..b5) of CMX, executed with both modality streams in
every kernel launch.

Parameter containers keep the reference module tree (``dual_segformer.py:19-528``), so
``state_dict`` keys match (``backbone.block2.3.attn.sr.weight``,
``backbone.extra_patch_embed1.proj.weight``, ...).  The containers hold parameters only;
``RGBXTransformer.run`` executes a stage for BOTH streams at once: the RGB module's
parameters are addressed through the ParamStore as (2, ...) stacked views that include
the ``extra_*`` twin, activations are (2, B*N, C) token-major tensors.
"""
from __future__ import annotations

import math
from typing import List, Optional

import torch
import torch.nn as nn

from ... import functions as F
from ... import streams
from ..net_utils import (FeatureRectifyModule, FeatureFusionModule, ImprovedFeatureRectifyModule,
                         ImprovedFeatureFusionModule, init_segformer)

MIT_SPECS = {
    "mit_b0": dict(embed_dims=[32, 64, 160, 256], depths=[2, 2, 2, 2]),
    "mit_b1": dict(embed_dims=[64, 128, 320, 512], depths=[2, 2, 2, 2]),
    "mit_b2": dict(embed_dims=[64, 128, 320, 512], depths=[3, 4, 6, 3]),
    "mit_b3": dict(embed_dims=[64, 128, 320, 512], depths=[3, 4, 18, 3]),
    "mit_b4": dict(embed_dims=[64, 128, 320, 512], depths=[3, 8, 27, 3]),
    "mit_b5": dict(embed_dims=[64, 128, 320, 512], depths=[3, 6, 40, 3]),
}
NUM_HEADS = [1, 2, 5, 8]
SR_RATIOS = [8, 4, 2, 1]
MLP_RATIO = 4


def drop_path_probs(depths: List[int], rate: float):
    """Per stage: (rgb_probs, x_probs) per block.  Reproduces dual_segformer.py:249-311,
    including the stage-2 indexing (block2[i] -> dpr[cur], extra_block2[i] -> dpr[cur+1])."""
    dpr = [x.item() for x in torch.linspace(0, rate, sum(depths))]
    out, cur = [], 0
    for s, d in enumerate(depths):
        if s == 1:
            out.append(([dpr[cur]] * d, [dpr[cur + 1]] * d))
        else:
            p = [dpr[cur + i] for i in range(d)]
            out.append((p, list(p)))
        cur += d
    return out


class DWConv(nn.Module):                          # dual_segformer.py:19-33
    def __init__(self, dim):
        super().__init__()
        self.dwconv = nn.Conv2d(dim, dim, 3, 1, 1, bias=True, groups=dim)


class Mlp(nn.Module):                             # dual_segformer.py:36-74
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.dwconv = DWConv(hidden)
        self.fc2 = nn.Linear(hidden, dim)


class Attention(nn.Module):                       # dual_segformer.py:77-138
    def __init__(self, dim, num_heads, sr_ratio):
        super().__init__()
        self.num_heads = num_heads
        self.q = nn.Linear(dim, dim, bias=True)
        self.kv = nn.Linear(dim, 2 * dim, bias=True)
        self.proj = nn.Linear(dim, dim)
        self.sr_ratio = sr_ratio
        if sr_ratio > 1:
            self.sr = nn.Conv2d(dim, dim, sr_ratio, sr_ratio)
            self.norm = nn.LayerNorm(dim)


class Block(nn.Module):                           # dual_segformer.py:141-180
    def __init__(self, dim, num_heads, sr_ratio, drop_path):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=1e-6)
        self.attn = Attention(dim, num_heads, sr_ratio)
        self.drop_path_prob = drop_path
        self.norm2 = nn.LayerNorm(dim, eps=1e-6)
        self.mlp = Mlp(dim, dim * MLP_RATIO)


class OverlapPatchEmbed(nn.Module):               # dual_segformer.py:183-225
    def __init__(self, patch_size, stride, in_chans, embed_dim):
        super().__init__()
        self.proj = nn.Conv2d(in_chans, embed_dim, patch_size, stride, patch_size // 2)
        self.norm = nn.LayerNorm(embed_dim)
        self.stride = stride
        self.pad = patch_size // 2


def _conv_bn_relu(cin, cout, k=1, rate=1):
    """Bias-free conv (3x3: dilation = padding = rate), plain BatchNorm2d, ReLU: every unit of the eASPP neck."""
    return nn.Sequential(nn.Conv2d(cin, cout, k, padding=rate if k > 1 else 0, dilation=rate if k > 1 else 1,
                                   bias=False), nn.BatchNorm2d(cout), nn.ReLU(True))


class ASPPConv(nn.Module):                        # dual_segformer_w_ef_aspp.py:18-28
    def __init__(self, channels, rate):
        super().__init__()
        self.block = _conv_bn_relu(channels, channels, 3, rate)


class AsppPooling(nn.Module):                     # dual_segformer_w_ef_aspp.py:31-45
    def __init__(self, cin, cout):
        super().__init__()
        self.gap = nn.Sequential(nn.AdaptiveAvgPool2d(1), *_conv_bn_relu(cin, cout))


class eASPP(nn.Module):                           # dual_segformer_w_ef_aspp.py:48-157
    """The "efficient ASPP" neck on the stage-4 fused map: a 1x1 entry, three branches 1x1 -> 3 dilated 3x3 -> 1x1 at
    width 64 (one rate each), an image-pooling branch, and a 1x1 projection of their concat with an elementwise
    Dropout(0.5).  Every norm is a plain nn.BatchNorm2d (never SyncBatchNorm, as in the reference); registration names
    are the reference's, so its ``backbone.single_aspp.*`` keys load.

    ``run`` in launches (training, M = B h w <= 600 rows, so every BatchNorm is one launch each way): the four 1x1
    convs that read x as ONE multi GEMM, each depth level of the three branches as ONE grouped dilated convolution
    (functions.DilatedConv3F), the three exit 1x1 convs as ONE multi GEMM, the pooled branch (pool, tiny linear, BN),
    one launch that assembles the concat buffer with the pooled row broadcast, the projection GEMM, the dropout
    mask, and the 18 BatchNorm + ReLU launches (the last one applies the dropout scale): 28 forward."""
    reduce_dim, middle_dim = 64, 256

    def __init__(self, channels, atrous_rates=(12, 24, 36)):
        super().__init__()
        r, m = self.reduce_dim, self.middle_dim
        self.input_conv = _conv_bn_relu(channels, m)
        for i, rate in enumerate(atrous_rates):
            setattr(self, f"branch{i + 1}", nn.ModuleList(
                [_conv_bn_relu(channels, r)] + [ASPPConv(r, rate) for _ in range(3)] + [_conv_bn_relu(r, m)]))
        self.img_pooling = AsppPooling(channels, m)
        self.project = nn.Sequential(*_conv_bn_relu(5 * m, channels), nn.Dropout(0.5))

    def dropout_scale(self, n, device, mask=None):
        """project's Dropout as F.batchnorm's elementwise dscale (n = rows * channels values): ``mask`` (0/1, any
        shape of n elements) forced, else drawn on the device from a seed and a device-side step counter, so a replayed
        HIP graph draws a fresh mask without a host copy.  The counter is made at the first call, which must be an
        eager one: inside a graph capture it raises."""
        p = self.project[3].p
        if p <= 0:
            return None
        if mask is not None:
            return (mask.to(device=device, dtype=torch.float32).reshape(-1) / (1 - p)).contiguous()
        device = torch.device(device)
        st = self.__dict__.get("_mask_state")
        if st is None or st[1].device.type != device.type or device.index not in (None, st[1].device.index):
            if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
                # made inside a capture the counter would live in the graph's pool, and its zero fill would be
                # replayed: every replay would draw the first mask again
                raise RuntimeError("eASPP: the dropout mask's device step counter must exist before a graph capture: "
                                   "run one eager training step first")
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())       # from torch's host generator
            st = self.__dict__["_mask_state"] = (seed, torch.zeros(2, dtype=torch.int64, device=device))
        return F.easpp_dropout_scale(st, n, p, device)

    def run(self, store, x, B, h, w, training, mask=None):
        """x (B*h*w, C) tokens of the fused map -> the neck's output, same shape.  mask: a forced (B, h, w, C) 0/1
        dropout mask (training only; None: drawn on the device)."""
        M, N = B * h * w, h * w
        if training and B == 1:
            raise ValueError("eASPP: training needs more than 1 image per batch: the pooled branch's BatchNorm sees "
                             "one value per channel (as torch.nn.BatchNorm2d refuses)")
        br = (self.branch1, self.branch2, self.branch3)

        def unit(seq, t, **kw):
            return F.batchnorm(store, seq[1], t, training, act="relu", **kw)

        xg = x.view(1, M, -1)
        ys = F.glinear_multi(store, [(u[0].weight, None, xg) for u in (self.input_conv, *(b[0] for b in br))])
        x_in = unit(self.input_conv, ys[0].view(M, -1))
        t = [unit(b[0], y.view(M, -1)) for b, y in zip(br, ys[1:])]
        for d in (1, 2, 3):
            t = F.dilated_conv3(store, [b[d].block[0] for b in br], t, B, h, w)
            t = [unit(b[d].block, y) for b, y in zip(br, t)]
        ys = F.glinear_multi(store, [(b[4][0].weight, None, y.view(1, M, -1)) for b, y in zip(br, t)])
        outs = [unit(b[4], y.view(M, -1)) for b, y in zip(br, ys)]
        gap = self.img_pooling.gap
        pool = F.batchnorm(store, gap[2], F.pooled_conv(store, gap[1], x, B, N), training, act="relu")
        cat = F.EasppConcatF.apply(x_in, *outs, pool, B, N)
        y = F.glinear(store, self.project[0].weight, None, cat.view(1, M, -1)).view(M, -1)
        scale = self.dropout_scale(y.numel(), y.device, mask) if training else None
        return unit(self.project, y, dscale=scale, rps=1)


class RGBXTransformer(nn.Module):                 # dual_segformer.py:228-446
    def __init__(self, embed_dims, depths, drop_path_rate=0.1, frm="FRM", ffm="FFM", aspp=False):
        super().__init__()
        self.embed_dims, self.depths = list(embed_dims), list(depths)
        self.dp = drop_path_probs(depths, drop_path_rate)
        cins = [3] + list(embed_dims[:3])
        for pre in ("", "extra_"):
            for s in range(4):
                k, st = (7, 4) if s == 0 else (3, 2)
                setattr(self, f"{pre}patch_embed{s + 1}", OverlapPatchEmbed(k, st, cins[s], embed_dims[s]))
        for s in range(4):
            for pre, probs in (("", self.dp[s][0]), ("extra_", self.dp[s][1])):
                setattr(self, f"{pre}block{s + 1}", nn.ModuleList(
                    [Block(embed_dims[s], NUM_HEADS[s], SR_RATIOS[s], probs[i]) for i in range(depths[s])]))
                setattr(self, f"{pre}norm{s + 1}", nn.LayerNorm(embed_dims[s], eps=1e-6))
        # config.feature_rectify_module / feature_fusion_module (dual_segformer.py:316-340):
        # anything but 'FRM' / 'FFM' selects the improved variant, as in the reference
        rect = FeatureRectifyModule if frm == "FRM" else ImprovedFeatureRectifyModule
        fuse = FeatureFusionModule if ffm == "FFM" else ImprovedFeatureFusionModule
        self.FRMs = nn.ModuleList([rect(d) for d in embed_dims])
        self.FFMs = nn.ModuleList([fuse(d, NUM_HEADS[s]) for s, d in enumerate(embed_dims)])
        if aspp:    # the mit_b*_w_ef_aspp family (dual_segformer_w_ef_aspp.py:477): one neck, on the stage-4 fused map
            self.single_aspp = eASPP(embed_dims[3], atrous_rates=(12, 24, 36))
        self.apply(init_segformer)

    # ------------------------------------------------------------------------ execution
    def drop_path_keep_probs(self):
        """(n_blocks_total, 2) keep probabilities in execution order (stage, block)."""
        rows = []
        for s in range(4):
            for i in range(self.depths[s]):
                rows.append((1.0 - self.dp[s][0][i], 1.0 - self.dp[s][1][i]))
        return rows

    def run_block(self, store, blk: Block, x, B, H, W, s_attn, s_mlp, prev=(None, None), tail=None,
                  next_norm=None):
        """One Block (dual_segformer.py:166-180) for both streams.  ``prev`` = (DropPath scale,
        GradTap) of the residual branch that produced ``x`` (the previous block's fc2): norm1's
        backward writes that branch's scaled gradient.  ``tail``: the LNTail of norm1 when the
        producer of x normalised it in its launch; ``next_norm``: the norm that consumes this
        block's output (the next block's norm1 or the stage norm), computed in fc2's launch.
        Returns (x_out, (s_mlp, tap), LNTail of next_norm or None) for the next consumer of x_out."""
        G, M, C = x.shape
        N = H * W
        a = blk.attn
        # norm1 also passes x through for the attention residual: its backward sums both gradients
        # (q and the SR path read norm1's output through separate handles: the norm's backward
        # sums their gradients on load)
        # norm1's backward rides on the SR conv's input-gradient launch (C 64 / 128, exact patches)
        stap = F.DgradTap() if (a.sr_ratio > 1 and F.ln_bwd_fusable(x, (H, W, a.sr_ratio))) else None
        h, h2, xr = F.layernorm_res(store, blk.norm1, x, G, scale=prev[0], rps=N, tap=prev[1], tail=tail, dtap=stap)

        if a.sr_ratio > 1:
            xs, Hk, Wk = F.conv(store, a.sr, h2, G, G * B, H, W, C, a.sr_ratio, 0, dtap=stap)
            xs, Nk = F.layernorm(store, a.norm, xs, G), Hk * Wk
        else:
            xs, Nk = h2, N
        # q and kv as ONE GEMM launch (and their input gradients as another)
        q, kv = F.glinear_multi(store, [(a.q.weight, a.q.bias, h), (a.kv.weight, a.kv.bias, xs)])
        o = F.SRAttentionF.apply(q, kv, G * B, N, Nk, a.num_heads, C // a.num_heads)
        # x + drop_path(proj(o)): residual and DropPath scale fused into the proj GEMM epilogue
        tap_a = F.GradTap() if s_attn is not None else None
        t2 = F.LNTail(blk.norm2)
        x = F.glinear(store, a.proj.weight, a.proj.bias, o, res=xr, rscale=s_attn, rps=N, tap=tap_a, ln_tail=t2)
        # norm2's backward rides on fc1's dgrad launch (C <= 128): fc1 hands (dz, W1) over
        ltap = F.DgradTap() if F.ln_bwd_fusable(x) else None
        h, _, xr = F.layernorm_res(store, blk.norm2, x, G, scale=s_attn, rps=N, tap=tap_a, tail=t2, dtap=ltap)
        tap_m = F.GradTap() if s_mlp is not None else None
        tn = F.LNTail(next_norm) if next_norm is not None else None
        # fc1 -> DWConv + GELU -> fc2 (+ residual); at C 64 / 128 fc1 and fc2's input gradient run inside
        # the depthwise kernels (F.MlpF)
        x = F.mlp(store, blk.mlp, h, G * B, B, H, W, res=xr, rscale=s_mlp, rps=N, tap=tap_m, ln_tail=tn,
                  dgrad_tap=ltap)
        return x, (s_mlp, tap_m), tn

    def run(self, store, images, B, H, W, training, dp_scales: Optional[torch.Tensor], bn_group=None, aspp_mask=None):
        """images: (2*B, 3, H, W) fp32 NCHW (RGB batch then X batch), or the pair of (B, 3, H, W)
        batches (rgb, modal_x) read by the stage-1 im2col in place.
        dp_scales: (n_blocks_total, 2, 2*? ) per-block (attn, mlp) per-sample scales or None.
        aspp_mask: a forced dropout mask of the eASPP neck (eASPP.run), for the backbones that have one.
        Returns the 4 fused maps [(B*N_s, C_s) tokens] and their grids."""
        neck = getattr(self, "single_aspp", None)

        def fuse(s, r, Hc, Wc):
            o = self.FFMs[s].run(store, r, B, Hc, Wc, training)
            if s == 3 and neck is not None:      # :583-585, on the stream that produced the fused map
                o = neck.run(store, o, B, Hc, Wc, training, mask=aspp_mask)
            return o

        G = 2
        x2 = None
        if isinstance(images, (tuple, list)):
            x, x2 = images
        else:
            x = images
        outs, grids = [], []
        bi = 0
        Hc, Wc, Cin = H, W, 3
        sync = getattr(self, "grad_sync", None)     # dist.BucketedGradSync (data parallel) or None
        main = torch.cuda.current_stream() if x.is_cuda else None
        side = streams.ffm_stream(main.device) if (main is not None and streams.FFM_SIDE) else None
        for s in range(4):
            pe = getattr(self, f"patch_embed{s + 1}")
            if sync is not None and s > 0 and x.requires_grad:
                # the gradient of this stage's input exists once the backward has passed the
                # stage (segment 3 - s): its gradients can be all-reduced while stages < s run
                x.register_hook(sync.segment_hook(3 - s))
            if s == 0:      # conv on the NCHW images + LayerNorm in one launch where eligible
                x, Ho, Wo = F.patch_embed1(store, pe, x, G, G * B, Hc, Wc, x2=x2)
            else:
                x, Ho, Wo = F.conv(store, pe.proj, x, G, G * B, Hc, Wc, Cin, pe.stride, pe.pad)
                x = F.layernorm(store, pe.norm, x, G)
            Hc, Wc, Cin = Ho, Wo, self.embed_dims[s]
            prev = (None, None)
            blocks = getattr(self, f"block{s + 1}")
            snorm = getattr(self, f"norm{s + 1}")
            tail = None
            for i, blk in enumerate(blocks):
                sa = sm = None
                if dp_scales is not None:
                    sa, sm = dp_scales[bi, 0], dp_scales[bi, 1]
                nxt = blocks[i + 1].norm1 if i + 1 < len(blocks) else snorm
                x, prev, tail = self.run_block(store, blk, x, B, Hc, Wc, sa, sm, prev, tail=tail, next_norm=nxt)
                bi += 1
            # stage norm: its backward also writes the last block's DropPath-scaled gradient
            x, _, _ = F.layernorm_res(store, snorm, x, G, scale=prev[0], rps=Hc * Wc, tap=prev[1], tail=tail)
            C = self.embed_dims[s]
            fr = self.FRMs[s]
            if isinstance(fr, ImprovedFeatureRectifyModule):
                r = rn = fr.rectify(store, x.view(G, B, Hc * Wc, C), training)
            else:
                r, rn = F.frm(store, fr, x.view(G, B, Hc * Wc, C))     # rn: the next stage's handle
            if side is not None:
                # FFM_s only feeds the decoder: run it beside stage s + 1 on the side stream
                # (its backward then runs there too, beside the encoder's backward)
                side.wait_stream(main)
                r.record_stream(side)
                with torch.cuda.stream(side):
                    outs.append(fuse(s, r, Hc, Wc))
            else:
                outs.append(fuse(s, r, Hc, Wc))
            grids.append((Hc, Wc))
            x = rn.view(G, B * Hc * Wc, C)
        if side is not None:
            main.wait_stream(side)
            for o in outs:
                o.record_stream(main)
        return outs, grids


class mit_b0(RGBXTransformer):
    def __init__(self, fuse_cfg=None, frm="FRM", ffm="FFM", **kwargs):
        super().__init__(**MIT_SPECS["mit_b0"], drop_path_rate=0.1, frm=frm, ffm=ffm)


class mit_b1(RGBXTransformer):
    def __init__(self, fuse_cfg=None, frm="FRM", ffm="FFM", **kwargs):
        super().__init__(**MIT_SPECS["mit_b1"], drop_path_rate=0.1, frm=frm, ffm=ffm)


class mit_b2(RGBXTransformer):
    def __init__(self, fuse_cfg=None, frm="FRM", ffm="FFM", **kwargs):
        super().__init__(**MIT_SPECS["mit_b2"], drop_path_rate=0.1, frm=frm, ffm=ffm)


class mit_b3(RGBXTransformer):
    def __init__(self, fuse_cfg=None, frm="FRM", ffm="FFM", **kwargs):
        super().__init__(**MIT_SPECS["mit_b3"], drop_path_rate=0.1, frm=frm, ffm=ffm)


class mit_b4(RGBXTransformer):
    def __init__(self, fuse_cfg=None, frm="FRM", ffm="FFM", **kwargs):
        super().__init__(**MIT_SPECS["mit_b4"], drop_path_rate=0.1, frm=frm, ffm=ffm)


class mit_b5(RGBXTransformer):
    def __init__(self, fuse_cfg=None, frm="FRM", ffm="FFM", **kwargs):
        super().__init__(**MIT_SPECS["mit_b5"], drop_path_rate=0.1, frm=frm, ffm=ffm)


BACKBONES = {"mit_b0": mit_b0, "mit_b1": mit_b1, "mit_b2": mit_b2, "mit_b3": mit_b3, "mit_b4": mit_b4,
             "mit_b5": mit_b5}


def _with_ef_aspp(name):
    """``name`` + "_w_ef_aspp" (config.py's backbone names of dual_segformer_w_ef_aspp.py): the same encoder with the
    eASPP neck on the stage-4 fused map.  Channels follow embed_dims, and mit_b1_w_ef_aspp is the real B1, as for the
    plain backbones (models/builder.py's docstring)."""
    spec = MIT_SPECS[name]

    class Net(RGBXTransformer):
        def __init__(self, fuse_cfg=None, frm="FRM", ffm="FFM", **kwargs):
            super().__init__(**spec, drop_path_rate=0.1, frm=frm, ffm=ffm, aspp=True)

    Net.__name__ = Net.__qualname__ = f"{name}_w_ef_aspp"
    return Net


for _name in list(MIT_SPECS):
    MIT_SPECS[f"{_name}_w_ef_aspp"] = MIT_SPECS[_name]
    BACKBONES[f"{_name}_w_ef_aspp"] = _with_ef_aspp(_name)


def load_dualpath_model(model: nn.Module, model_file):
    """Pretrained MiT weights duplicated into both streams (dual_segformer.py:449-480).
    ``model_file`` is a path (loaded with weights_only=True) or a state dict."""
    raw = torch.load(model_file, map_location="cpu", weights_only=True) if isinstance(model_file, str) \
        else model_file
    if "model" in raw:
        raw = raw["model"]
    sd = {}
    for k, v in raw.items():
        if "patch_embed" in k:
            sd[k] = v
            sd[k.replace("patch_embed", "extra_patch_embed")] = v
        elif "block" in k:
            sd[k] = v
            sd[k.replace("block", "extra_block")] = v
        elif "norm" in k:
            sd[k] = v
            sd[k.replace("norm", "extra_norm")] = v
    return model.load_state_dict(sd, strict=False)
