"""Algorithmic work of the CMX training step, counted op by op as the reference executes
it: every Linear, Conv2d (incl. depthwise and the SR
patchify), QK^T, PV, K^T V and Q ctx; no elementwise / norm / softmax / pool / interpolate.
FLOP = 2 * MAC; training = 3 x forward.  Reported roofline fractions use THIS count."""
from __future__ import annotations

from .models.encoders.dual_segformer import MIT_SPECS, NUM_HEADS, SR_RATIOS


def _grid(H, W, k, s, p):
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def easpp_macs(N, C) -> int:
    """The eASPP neck on an N-pixel, C-channel map (dual_segformer_w_ef_aspp.py:48-157): the four 1x1 convs that read
    it (256 + 3 * 64 outputs), nine dilated 3x3 64 -> 64 convs, three 64 -> 256 exits, the 1280 -> C projection, and
    the pooled branch's 1x1 conv on one pixel.  Taps that fall outside the map are counted, as the reference runs
    them."""
    return N * (C * 448 + 9 * 9 * 64 * 64 + 3 * 64 * 256 + 1280 * C) + C * 256


def deeplabv3plus_macs(N1, C1, N4, C4, K) -> int:
    """The DeepLabV3+ head (decoders/deeplabv3plus.py) on an N1-pixel, C1-channel stage-1 map and an N4-pixel,
    C4-channel stage-4 map: ASPP's 1x1 conv and three dilated 3x3 convs C4 -> 256 (all 27 taps, as the reference runs
    them), the pooled branch's 1x1 conv on one pixel, the 1280 -> 256 projection; the 3x3 C1 -> 48 projection, the 3x3
    304 -> 256 conv and the classifier on the stage-1 grid."""
    aspp = N4 * (C4 * 256 + 3 * 9 * C4 * 256 + 1280 * 256) + C4 * 256
    return aspp + N1 * (9 * C1 * 48 + 9 * 304 * 256 + 256 * K)


def uperhead_macs(grids, K, channels=512, pool_scales=(1, 2, 3, 6)) -> int:
    """The UPerNet head (decoders/UPernet.py) on the four stage maps ``grids`` = [(N_i pixels, C_i channels)] of one
    image: the four PPM 1x1 convs on their s x s pooled pixels, the 3x3 bottleneck (C4 + 4 channels) -> channels on
    the stage-4 grid, three 1x1 laterals, three 3x3 FPN convs, the 3x3 fpn_bottleneck 4 channels -> channels and the
    classifier on the stage-1 grid."""
    Ch = channels
    (N1, _), (N4, C4) = grids[0], grids[3]
    ppm = sum(s * s for s in pool_scales) * C4 * Ch + N4 * 9 * (C4 + len(pool_scales) * Ch) * Ch
    fpn = sum(N * (C * Ch + 9 * Ch * Ch) for N, C in grids[:3])
    return ppm + fpn + N1 * (9 * 4 * Ch * Ch + Ch * K)


def forward_macs_per_image(backbone="mit_b2", H=480, W=640, K=40, E=512, decoder="MLPDecoder") -> int:
    """decoder: "MLPDecoder" (the default; MLPDecoderpp's gate adds no counted op), "DeepLabV3Plus" or "UPerHead"
    (channels = 512, as the builder constructs it), the latter two without their auxiliary head."""
    dims, depths = MIT_SPECS[backbone]["embed_dims"], MIT_SPECS[backbone]["depths"]
    total = 0
    h, w = H, W
    cin = 3
    grids = []
    for s in range(4):
        k, st = (7, 4) if s == 0 else (3, 2)
        h, w = _grid(h, w, k, st, k // 2)
        N, C = h * w, dims[s]
        grids.append((N, C))
        pe = N * C * cin * k * k
        R = SR_RATIOS[s]
        if R > 1:
            hk, wk = _grid(h, w, R, R, 0)
            Nk = hk * wk
        else:
            Nk = N
        blk = N * C * C + 2 * Nk * C * C + 2 * N * Nk * C + N * C * C + 8 * N * C * C + 36 * N * C
        if R > 1:
            blk += Nk * R * R * C * C
        total += 2 * (pe + depths[s] * blk)                    # both modality streams
        d = C // NUM_HEADS[s]
        total += 2 * N * C * C + 2 * N * C + 24 * C * C        # FRM
        total += 17 * N * C * C + 4 * N * C * d + 9 * N * C    # FFM
        if s == 3 and backbone.endswith("_w_ef_aspp"):
            total += easpp_macs(N, C)
        cin = C
    N1 = grids[0][0]
    if decoder == "DeepLabV3Plus":
        return total + deeplabv3plus_macs(N1, grids[0][1], grids[3][0], grids[3][1], K)
    if decoder == "UPerHead":
        return total + uperhead_macs(grids, K)
    total += sum(N * C * E for N, C in grids) + N1 * 4 * E * E + N1 * E * K
    return total


def train_flops_per_image(**kw) -> float:
    return 6.0 * forward_macs_per_image(**kw)


if __name__ == "__main__":
    m = forward_macs_per_image()
    print(m, train_flops_per_image() / 1e9, "GFLOP/img")
