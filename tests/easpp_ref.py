"""The eASPP neck of the mit_b*_w_ef_aspp backbones (models/encoders/dual_segformer_w_ef_aspp.py:18-157, 477, 583-585
of the reference) restated in plain PyTorch for the tests: the reference's registration names (so the 108 keys under
``backbone.single_aspp.`` are the reference's), any floating dtype including fp64, and a Dropout whose keep mask can be
set.  ``NeckBackbone`` is the oracle's dual-stream encoder with the neck applied to the stage-4 fused map, so that
``oracle.cmx_ref.EncoderDecoder`` can carry it; ``ref_model`` builds that oracle.
"""
import torch
import torch.nn as nn

from oracle.cmx_ref import CMXConfig, EncoderDecoder, MIT_SPECS, RGBXTransformer, segformer_init

RATES = (12, 24, 36)
REDUCE, MIDDLE, P_DROP = 64, 256, 0.5


class MaskedDropout(nn.Module):
    """nn.Dropout(p), elementwise, with an injectable keep mask of the input's shape (NCHW)."""

    def __init__(self, p):
        super().__init__()
        self.p = p
        self.mask = None

    def forward(self, x):
        if not self.training or self.p == 0.0:
            return x
        m = self.mask if self.mask is not None else torch.bernoulli(torch.full(x.shape, 1 - self.p, device=x.device))
        return x * m.to(x.dtype) / (1 - self.p)


def unit(cin, cout, k=1, rate=1):
    return [nn.Conv2d(cin, cout, k, padding=rate * (k // 2), dilation=rate, bias=False), nn.BatchNorm2d(cout),
            nn.ReLU()]


class ASPPConv(nn.Module):
    def __init__(self, rate):
        super().__init__()
        self.block = nn.Sequential(*unit(REDUCE, REDUCE, 3, rate))

    def forward(self, x):
        return self.block(x)


class AsppPooling(nn.Module):
    def __init__(self, cin):
        super().__init__()
        self.gap = nn.Sequential(nn.AdaptiveAvgPool2d(1), *unit(cin, MIDDLE))

    def forward(self, x):
        # bilinear, align_corners=True, from a 1 x 1 map: every output pixel is that one value
        return self.gap(x).expand(-1, -1, *x.shape[2:])


class EASPPRef(nn.Module):
    def __init__(self, channels, rates=RATES):
        super().__init__()
        self.input_conv = nn.Sequential(*unit(channels, MIDDLE))
        for i, r in enumerate(rates):
            setattr(self, f"branch{i + 1}", nn.ModuleList(
                [nn.Sequential(*unit(channels, REDUCE)), ASPPConv(r), ASPPConv(r), ASPPConv(r),
                 nn.Sequential(*unit(REDUCE, MIDDLE))]))
        self.img_pooling = AsppPooling(channels)
        self.project = nn.Sequential(*unit(5 * MIDDLE, channels), MaskedDropout(P_DROP))
        self.apply(segformer_init)          # the backbone's _init_weights: conv normal(0, sqrt(2 / fan_out)), BN 1 / 0

    def forward(self, x):
        parts = [self.input_conv(x)]
        for branch in (self.branch1, self.branch2, self.branch3):
            t = x
            for m in branch:
                t = m(t)
            parts.append(t)
        parts.append(self.img_pooling(x))
        return self.project(torch.cat(parts, 1))


class NeckBackbone(RGBXTransformer):
    def __init__(self, embed_dims, *args, **kw):
        super().__init__(embed_dims, *args, **kw)
        self.single_aspp = EASPPRef(embed_dims[3])

    def forward(self, x_rgb, x_e, return_stages=False):
        outs, stages = super().forward(x_rgb, x_e, return_stages=True)
        outs[3] = self.single_aspp(outs[3])
        return (outs, stages) if return_stages else outs


def ref_model(backbone="mit_b0", **cfg):
    """oracle.cmx_ref.EncoderDecoder for ``backbone`` + "_w_ef_aspp" (fp32; the caller seeds torch first)."""
    c = CMXConfig(backbone=backbone, **cfg)
    ref = EncoderDecoder(c)
    spec = MIT_SPECS[backbone]
    ref.backbone = NeckBackbone(spec["embed_dims"], spec["depths"], c.drop_path_rate, c.feature_rectify_module,
                                c.feature_fusion_module)
    return ref


def jitter(neck, g, dtype=torch.float32):
    """Non-trivial BN affine parameters and running statistics, then every parameter rounded to ``dtype`` (values both
    sides can store)."""
    with torch.no_grad():
        for m in neck.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.weight.add_(0.1 * torch.randn(m.weight.shape, generator=g))
                m.bias.add_(0.1 * torch.randn(m.bias.shape, generator=g))
                m.running_mean.copy_(torch.rand(m.running_mean.shape, generator=g) * 0.2 - 0.1)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)
        for p in neck.parameters():
            p.copy_(p.to(dtype))
    return neck


def settle_kinks(neck, x, training, tol=1e-4, step=1e-3):
    """Move BatchNorm biases of ``neck`` (fp32, in place) until no ReLU of the neck has an input within ``tol`` of
    zero for the input x (NCHW, fp64) in the given mode, as computed in fp64.

    Why: a max-abs comparison of gradients against fp64 means nothing at an element whose pre-activation is below the
    rounding error of its own computation -- which side of zero it lands on is a coin toss for ANY fp32
    implementation, and the losing side changes a whole gradient path by O(1e-2).  At the sizes tested here (about
    2e6 pre-activations of unit scale) every random draw has a few such elements.  A bias shift moves one channel of
    one BatchNorm and nothing upstream of it, so the layers are settled in execution order (= registration order),
    re-running the fp64 forward after each change.  With no pre-activation within 1e-4 of zero, an implementation that
    is within the 1e-5 the tests allow cannot flip a ReLU, and neither can the fp32 yardstick."""
    import copy
    ref = copy.deepcopy(neck).double().train(training)
    pairs = [(a, b) for a, b in zip(neck.modules(), ref.modules()) if isinstance(a, nn.BatchNorm2d)]
    seen = {}
    hooks = [b.register_forward_hook(lambda m, i, o: seen.__setitem__(m, o.detach())) for _, b in pairs]
    with torch.no_grad():
        for bn, rbn in pairs:
            for _ in range(100):
                ref(x)
                near = (seen[rbn].abs() < tol).transpose(0, 1).flatten(1).any(1)
                if not bool(near.any()):
                    break
                bn.bias[near] += step
                rbn.bias.copy_(bn.bias.double())
            else:
                raise AssertionError("settle_kinks: a channel keeps a pre-activation near zero")
    for h in hooks:
        h.remove()
    return neck
