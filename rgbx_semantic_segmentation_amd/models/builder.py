"""Drop-in ``EncoderDecoder`` (reference: models/builder.py:14-253) on MI355X kernels.

API kept from the reference:
  ``EncoderDecoder(cfg, criterion=nn.CrossEntropyLoss(reduction='mean', ignore_index=255),
                   norm_layer=nn.BatchNorm2d)``; ``criterion`` may also carry a class ``weight``, or be
  ``utils.loss_opr.FocalLoss`` / ``FocalLoss2d`` or the CE_Focal tuple ``(CrossEntropyLoss, FocalLoss)``
  (train.py:70-88); anything else raises ``NotImplementedError``
  attributes ``backbone``, ``decode_head``, ``criterion``, ``channels``, ``aux_head = None``;
  ``forward(rgb, modal_x, label=None)`` -> 0-dim loss (with autograd graph) if ``label`` is
  given, else fp32 logits (B, K, H, W); ``encode_decode``; ``init_weights``; ``state_dict``
  keys identical to the reference.

Differences by design:
  * ``model.cuda()`` / ``model.to(device)`` flattens the parameters into a ParamStore
    (one fp32 buffer + gradient buffer + bf16 / fp16 shadow); parameters remain ``nn.Parameter``
    views with reference shapes.  There is no CPU execution path: forward on a model that
    was not moved to a GPU raises.
  * Decoder input channels come from the encoder's ``embed_dims`` (the reference's
    hard-coded [96,192,384,768] for mit_b4/b5, builder.py:66-75, cannot run; its mit_b1
    entry builds mit_b0, :84-87).
  * ``mit_b{0..5}_w_ef_aspp`` (dual_segformer_w_ef_aspp.py): the same encoders with the eASPP neck on the stage-4
    fused map; the same two differences hold (its hard-coded [96,192,384,768] and its b1 -> b0), FRM / FFM stay
    selectable, and training with one image per batch raises ValueError (the pooled branch's BatchNorm, as in torch).
    The pooled branch's 1x1 conv runs on cmx_small_linear, which takes at most 8 rows: with the neck a batch is at
    most 8 images per GPU (more is refused with the library's shape error, not computed another way).  The random
    mask of the neck's Dropout keeps a step counter on the device; it is made by the first training forward, which
    must be an eager one (inside a graph capture it raises).
    ``forced_masks["aspp_dropout"]``: an optional (B, h, w, C4) 0/1 mask of the neck's Dropout for tests.
  * ``cfg.decoder = "FCNHead"``: the reference's fallback branch (builder.py:186-189, FCN-32s: decoders.fcnhead.FCNHead
    on the stage-4 map) under an explicit name; the other names of builder.py:154-189 stay refused.  ``cfg.aux_head``
    (default False; ``cfg.aux_rate``, default 0.4): the auxiliary FCNHead on the stage-3 map of builder.py:167-170 beside
    ANY decoder (the reference builds it only beside UPernet / DeepLabV3+); with a label the loss is main + aux_rate *
    criterion(aux logits upsampled), in train and eval mode, and without one the head is not run.  A head that is not at
    1/4 resolution takes its loss through functions.UpsampleScaledLossF: plain and class-weighted CrossEntropyLoss,
    FocalLoss, FocalLoss2d and, for the decode head only, CE_Focal; Dice, DiceCE and OHEM with such a head, and CE_Focal
    with aux_head (the reference would call the tuple), raise NotImplementedError at construction.
  * ``cfg.decoder = "DeepLabV3Plus"``: the reference's ``deeplabv3+`` branch (builder.py:172-179,
    decoders.deeplabv3plus.DeepLabV3Plus) under its class name; the reference's own spelling stays refused, as do
    ``UPernet`` and ``mask2former``.  Its logits are at 1/4 resolution, so every criterion above applies to it.  As in the
    reference the auxiliary FCNHead is built beside it BY DEFAULT (``cfg.aux_head = False`` switches it off; Dice, DiceCE,
    OHEM and CE_Focal need that).  Training with one image per batch raises ValueError and a batch is at most 8 images
    per GPU (the pooled ASPP branch, as for the eASPP neck); the head's two elementwise Dropouts keep device step counters
    made by the first, eager training forward.  ``forced_masks["dlv3_aspp_dropout"]`` (B, h4, w4, 256) and
    ``forced_masks["dlv3_block_dropout"]`` (B, h1, w1, 256): optional 0/1 masks of those Dropouts for tests.
  * ``cfg.decoder = "UPerHead"``: the reference's ``UPernet`` branch (builder.py:163-170, decoders.UPernet.UPerHead with
    channels=512) under its class name; the reference's own spelling stays refused.  Logits at 1/4 resolution, the
    auxiliary FCNHead beside it BY DEFAULT, as for DeepLabV3Plus.  The forward values are the reference's; its in-place
    top-down sum makes the reference's own backward raise, so the gradient is that of the out-of-place sum
    (decoders/UPernet.py).  Training with one image per batch raises ValueError (the scale-1 pooling BatchNorm); the head
    adds no upper limit on the batch.
  * compute dtype: ``cfg.compute_dtype`` ("float32" | "bfloat16" | "float16"); defaults to
    float16 when ``cfg.use_mixed_precision`` (the reference's fp16 autocast switch,
    config.py:61, train.py:185-198: fp16 storage, fp32 accumulation, with dynamic loss scaling
    by optim.GradScaler), else float32.
  * ``backward`` writes parameter gradients straight into the flat gradient buffer
    (overwrite, not accumulate); use the package's ``FusedAdamW``.
"""
from __future__ import annotations

import logging
from typing import Optional

import torch
import torch.nn as nn

from .. import functions as F
from .. import kernels as K
from ..params import ParamStore
from .decoders import MLPDecoder, MLPDecoderpp
from .decoders.MLPDecoder import DecoderHead
from .decoders.UPernet import UPerHead
from .decoders.deeplabv3plus import DeepLabV3Plus
from .decoders.fcnhead import FCNHead
from .encoders.dual_segformer import BACKBONES, MIT_SPECS, load_dualpath_model

logger = logging.getLogger("cmx")

PE1_KPAD = 152  # 3*7*7 = 147 padded to a multiple of 8 (16-byte aligned GEMM rows)


def _get(cfg, name, default):
    if cfg is None:
        return default
    if isinstance(cfg, dict):
        return cfg.get(name, default)
    return getattr(cfg, name, default)


def backward_segment(name: str) -> int:
    """Backward-completion segment of a parameter: 0 = decode head + stage 4 (done first),
    1 = stage 3, 2 = stage 2, 3 = stage 1.  A stage's patch embed, blocks, norm, FRM and FFM
    all have their final gradients once the backward has passed that stage's patch embed."""
    import re
    if name.startswith("decode_head.") or name.startswith("aux_head."):
        return 0
    m = re.match(r"backbone\.(?:extra_)?(?:patch_embed|block|norm)(\d)\.", name)
    if m:
        return 4 - int(m.group(1))
    m = re.match(r"backbone\.(?:FRMs|FFMs)\.(\d)\.", name)
    if m:
        return 3 - int(m.group(1))
    return 0


# cfg.decoder (builder.py:154-161 of the reference) -> decode head class
# "FCNHead": the reference's fallback branch (builder.py:186-189, FCN-32s on the stage-4 map) under an explicit name
# "DeepLabV3Plus": the reference's 'deeplabv3+' branch (builder.py:172-179) under its class name
# "UPerHead": the reference's 'UPernet' branch (builder.py:163-170) under its class name
DECODERS = {"MLPDecoder": MLPDecoder.DecoderHead, "MLPDecoderpp": MLPDecoderpp.DecoderHead, "FCNHead": FCNHead,
            "DeepLabV3Plus": DeepLabV3Plus, "UPerHead": UPerHead}
AUX_BY_DEFAULT = ("DeepLabV3Plus", "UPerHead")   # builder.py:163-179 builds the auxiliary head beside these decoders
AUX_INDEX, AUX_RATE = 2, 0.4      # builder.py:168-169

SUPPORTED_CRITERIA = ("nn.CrossEntropyLoss(reduction='mean'[, weight=w]), FocalLoss(reduction='mean', gamma == 0 or "
                      "gamma >= 1), FocalLoss2d(reduction='mean'[, weight=w]), DiceLoss(reduction='mean'), "
                      "DiceCELoss(reduction='mean'), ProbOhemCrossEntropy2d(reduction='mean') and CE_Focal = the tuple "
                      "(nn.CrossEntropyLoss(reduction='mean'), FocalLoss(...))")


class DiceSpec(tuple):
    """UpsampleDiceF's (ce_scale, dice_scale, smooth): a type of its own, so that forward tells it
    from UpsampleLossF's 5-tuple."""
    __slots__ = ()


class OhemSpec(tuple):
    """UpsampleOhemF's (thresh, min_kept): a type of its own, as DiceSpec."""
    __slots__ = ()


def _loss_plan(criterion):
    """(ignore_index, spec, class weight) of a supported criterion (train.py:70-88), else
    NotImplementedError naming the supported set.  spec None: plain CrossEntropyLoss, the
    UpsampleCEF path; a DiceSpec: DiceLoss / DiceCELoss, the UpsampleDiceF path; an OhemSpec:
    ProbOhemCrossEntropy2d, the UpsampleOhemF path; otherwise UpsampleLossF's (kind, gamma, alpha,
    ce_scale, focal_scale)."""
    from ..utils.loss_opr import (CE_FOCAL_WEIGHT, DiceCELoss, DiceLoss, FocalLoss, FocalLoss2d,
                                  ProbOhemCrossEntropy2d, check_focal_gamma)

    def refuse(why):
        raise NotImplementedError(f"criterion: {why}; on the hot path: {SUPPORTED_CRITERIA}")

    def plain_ce(c):
        if not isinstance(c, nn.CrossEntropyLoss):
            return False
        if c.reduction != "mean":
            refuse(f"CrossEntropyLoss(reduction={c.reduction!r})")
        if c.label_smoothing != 0.0:
            refuse("CrossEntropyLoss with label_smoothing")
        return True

    def focal(c):
        if c.reduction != "mean":
            refuse(f"FocalLoss(reduction={c.reduction!r})")
        return check_focal_gamma(c.gamma), float(c.alpha)     # ValueError on 0 < gamma < 1

    if plain_ce(criterion):
        if criterion.weight is None:
            return int(criterion.ignore_index), None, None
        return int(criterion.ignore_index), (F.LOSS_WCE, 0.0, 0.0, 1.0, 0.0), criterion.weight
    if isinstance(criterion, FocalLoss):
        gamma, alpha = focal(criterion)
        return int(criterion.ignore_label), (F.LOSS_FOCAL, gamma, alpha, 0.0, 1.0), None
    if isinstance(criterion, FocalLoss2d):
        if criterion.loss.reduction != "mean":
            refuse(f"FocalLoss2d(reduction={criterion.loss.reduction!r})")
        return int(criterion.loss.ignore_index), (F.LOSS_FOCAL2D, 0.0, 0.0, 1.0, 0.0), criterion.loss.weight
    def dice(c):
        if c.reduction != "mean":
            refuse(f"DiceLoss(reduction={c.reduction!r})")
        if not float(c.smooth) > 0:
            refuse(f"DiceLoss(smooth={c.smooth!r})")
        return float(c.smooth)

    if isinstance(criterion, DiceLoss):
        return int(criterion.ignore_index), DiceSpec((0.0, 1.0, dice(criterion))), None
    if isinstance(criterion, DiceCELoss):
        smooth, alpha = dice(criterion.dice), float(criterion.alpha)
        if not plain_ce(criterion.ce) or criterion.ce.weight is not None:
            refuse("DiceCELoss whose ce is not an unweighted CrossEntropyLoss")
        if int(criterion.ce.ignore_index) != int(criterion.dice.ignore_index):
            refuse("DiceCELoss whose two terms ignore different labels")
        if not 0.0 <= alpha <= 1.0:
            refuse(f"DiceCELoss(alpha={criterion.alpha!r})")
        return int(criterion.ce.ignore_index), DiceSpec((1.0 - alpha, alpha, smooth)), None
    if isinstance(criterion, ProbOhemCrossEntropy2d):
        if criterion.reduction != "mean":
            refuse(f"ProbOhemCrossEntropy2d(reduction={criterion.reduction!r})")
        return int(criterion.ignore_label), OhemSpec((float(criterion.thresh), int(criterion.min_kept))), None
    if isinstance(criterion, (tuple, list)) and len(criterion) == 2 and isinstance(criterion[1], FocalLoss) \
            and plain_ce(criterion[0]):
        ce, fl = criterion
        if ce.weight is not None:
            refuse("CE_Focal with a class weight")
        if int(ce.ignore_index) != int(fl.ignore_label):
            refuse("CE_Focal whose two terms ignore different labels")
        gamma, alpha = focal(fl)
        # CE + 0.2 * Focal (builder.py:246-247).  Labels outside [0, K) other than the ignore value are
        # unsupported here: torch's CrossEntropyLoss asserts on them (the kernel clamps them, as FocalLoss)
        return int(ce.ignore_index), (F.LOSS_FOCAL, gamma, alpha, 1.0, CE_FOCAL_WEIGHT), None
    refuse(type(criterion).__name__)


def effective_aux(decoder, aux_head) -> bool:
    """Whether the auxiliary head is built: ``aux_head`` as configured (None: not set), else the decoder's default."""
    return bool(aux_head) if aux_head is not None else decoder in AUX_BY_DEFAULT


def check_head_criterion(criterion, decoder, aux_head):
    """A head whose logits are not at 1/4 resolution (the FCNHead decode head at 1/32, the auxiliary head at 1/16)
    takes its loss through UpsampleScaledLossF, which has the per-pixel criteria only: NotImplementedError naming the
    reason for the others.  ``aux_head``: the effective setting (effective_aux).  Needs no GPU (train.py calls it before
    any GPU work)."""
    if decoder != "FCNHead" and not aux_head:
        return
    _, spec, _ = _loss_plan(criterion)
    where = "decoder='FCNHead'" if decoder == "FCNHead" else "aux_head"
    if isinstance(spec, (DiceSpec, OhemSpec)):
        name = type(criterion).__name__
        raise NotImplementedError(f"criterion {name} with {where}: the fused upsample + loss at x16 / x32 has plain and "
                                  "class-weighted CrossEntropyLoss, FocalLoss, FocalLoss2d and (decode head only) "
                                  f"CE_Focal; {name} exists at x4 only" +
                                  (" (the decode head is at x4: use it on the main head alone, or set aux_head=False)"
                                   if decoder != "FCNHead" else ""))
    if aux_head and isinstance(criterion, (tuple, list)):
        raise NotImplementedError("criterion CE_Focal with aux_head: the auxiliary loss is aux_rate * criterion(aux "
                                  "logits, label), and the reference would call the tuple there (builder.py:250-251); "
                                  "use another criterion, or set aux_head=False")


class EncoderDecoder(nn.Module):
    # the forward is one stream-ordered sequence of library launches with no host sync: callers
    # may capture it in a HIP graph (the evaluator does, per crop-batch shape)
    cmx_capturable = True

    def __init__(self, cfg=None, criterion=None, norm_layer=nn.BatchNorm2d):
        super().__init__()
        backbone = _get(cfg, "backbone", "mit_b2")
        if backbone not in BACKBONES:
            raise NotImplementedError(f"backbone {backbone!r}: only the MiT family (mit_b0..b5, and mit_b0..b5 + "
                                      "'_w_ef_aspp') is on the CMX hot path")
        decoder = _get(cfg, "decoder", "MLPDecoder")
        if decoder not in DECODERS:
            raise NotImplementedError(f"decoder {decoder!r}: only MLPDecoder and MLPDecoderpp are on the CMX hot path" +
                                      (" (the DeepLabV3+ head is selected by its class name, decoder='DeepLabV3Plus')"
                                       if decoder == "deeplabv3+" else
                                       " (the UPerNet head is selected by its class name, decoder='UPerHead')"
                                       if decoder == "UPernet" else ""))
        # config.py:57-58 selects the rectify / fusion blocks (dual_segformer.py:316-329: 'FRM' / 'FFM'
        # the originals, any other value the improved IFRM / IFFM, as there)
        frm = _get(cfg, "feature_rectify_module", "FRM")
        ffm = _get(cfg, "feature_fusion_module", "FFM")
        if criterion is None:
            criterion = nn.CrossEntropyLoss(reduction="mean", ignore_index=int(_get(cfg, "background", 255)))
        self.cfg = cfg
        self.norm_layer = norm_layer
        self.criterion = criterion         # the object(s) as given, as the reference keeps them
        self.ignore_index, self._loss_spec, self._loss_weight = _loss_plan(criterion)
        self.backbone_name = backbone
        self.channels = list(MIT_SPECS[backbone]["embed_dims"])
        self.backbone = BACKBONES[backbone](norm_fuse=norm_layer, frm=frm, ffm=ffm)
        self.aux_head = None
        self.num_classes = int(_get(cfg, "num_classes", 40))
        aux = effective_aux(decoder, _get(cfg, "aux_head", None))
        check_head_criterion(criterion, decoder, aux)
        if decoder == "FCNHead":           # builder.py:186-189: logits on the stage-4 grid
            self.decode_head = FCNHead(in_channels=self.channels[-1], kernel_size=3, num_classes=self.num_classes,
                                       norm_layer=norm_layer)
            self.decode_head.out_index = 3
        elif decoder == "DeepLabV3Plus":   # builder.py:172-179: the reference's constructor, logits on the stage-1 grid
            self.decode_head = DeepLabV3Plus(in_channels=self.channels, num_classes=self.num_classes,
                                             norm_layer=norm_layer)
        elif decoder == "UPerHead":        # builder.py:163-166: the reference's constructor, logits on the stage-1 grid
            self.decode_head = UPerHead(in_channels=self.channels, num_classes=self.num_classes,
                                        norm_layer=norm_layer, channels=512)
        else:
            self.decode_head = DECODERS[decoder](in_channels=self.channels, num_classes=self.num_classes,
                                                 norm_layer=norm_layer,
                                                 embed_dim=int(_get(cfg, "decoder_embed_dim", 512)))
        if aux:
            # the auxiliary head of builder.py:167-170 (there only beside UPernet / DeepLabV3+, where it is the default
            # here too; cfg.aux_head is an extension that allows it beside every decoder): FCNHead on the stage-3 map,
            # logits at 1/16
            self.aux_head = FCNHead(self.channels[AUX_INDEX], num_classes=self.num_classes, norm_layer=norm_layer)
            self.aux_head.out_index = AUX_INDEX
            self.aux_index = AUX_INDEX
            self.aux_rate = float(_get(cfg, "aux_rate", AUX_RATE))
        self.bn_eps = float(_get(cfg, "bn_eps", 1e-3))
        self.bn_momentum = float(_get(cfg, "bn_momentum", 0.1))
        dt = _get(cfg, "compute_dtype", None)
        if dt is None:
            dt = "float16" if _get(cfg, "use_mixed_precision", False) else "float32"
        self.compute_dtype = {"float32": torch.float32, "fp32": torch.float32, "bfloat16": torch.bfloat16,
                              "bf16": torch.bfloat16, "float16": torch.float16, "fp16": torch.float16}[str(dt)]
        self.sync_bn = norm_layer is nn.SyncBatchNorm
        self.process_group = None
        # DDP's default (train.py:145-146): the BatchNorm running statistics of rank 0 are
        # broadcast at the start of every training forward when a process group is set
        self.broadcast_buffers = True
        self._bnbuf = None
        self.store: Optional[ParamStore] = None
        self.forced_masks = None
        self.init_weights(cfg, pretrained=_get(cfg, "pretrained_model", None))

    # ------------------------------------------------------------------ init / placement
    def init_weights(self, cfg, pretrained=None):
        """builder.py:199-210: optional MiT pretrained load + decoder init_weight."""
        if pretrained:
            logger.info("Loading pretrained model: %s", pretrained)
            load_dualpath_model(self.backbone, pretrained)
        heads = [self.decode_head] + ([self.aux_head] if self.aux_head is not None else [])    # builder.py:204-210
        for m in (m for head in heads for m in head.modules()):
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_in", nonlinearity="relu")
            elif isinstance(m, nn.BatchNorm2d):
                m.eps, m.momentum = self.bn_eps, self.bn_momentum
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        if self.store is not None:
            self.store.refresh_shadow()

    def setup(self, device=None, compute_dtype=None):
        """Move buffers to ``device`` and flatten parameters into the ParamStore."""
        device = torch.device(device if device is not None else "cuda")
        if device.type != "cuda":
            raise RuntimeError("EncoderDecoder runs only on the GPU through libcmx_hip.so (no CPU path)")
        if compute_dtype is not None:
            self.compute_dtype = compute_dtype
        for mod in self.modules():
            for k, b in list(mod._buffers.items()):
                if b is not None:
                    mod._buffers[k] = b.to(device)
        if self.store is None:
            self.store = ParamStore(self, device, self.compute_dtype,
                                    conv_pad={"backbone.patch_embed1.proj.weight": PE1_KPAD,
                                              "backbone.extra_patch_embed1.proj.weight": PE1_KPAD},
                                    segment_of=backward_segment)
        if self._loss_weight is not None:      # the class weights: moved once, outside any capture
            self._loss_weight = self._loss_weight.detach().to(device=device, dtype=torch.float32).contiguous()
            if self._loss_weight.numel() != self.num_classes:
                raise ValueError(f"criterion weight has {self._loss_weight.numel()} entries, num_classes is "
                                 f"{self.num_classes}")
        from .. import deferred
        deferred.reserve()          # pinned launch-record tables for captured backward passes
        # every BatchNorm's num_batches_tracked is a view into one counter: one increment per
        # training forward instead of one launch per BN
        bns = [m for m in self.modules() if isinstance(m, nn.modules.batchnorm._BatchNorm)
               and m.num_batches_tracked is not None]
        if bns and getattr(self, "_nbt", None) is None:
            cnt = torch.stack([m.num_batches_tracked.to(device) for m in bns]).contiguous()
            for i, m in enumerate(bns):
                m._buffers["num_batches_tracked"] = cnt[i]
                m._nbt_shared = True
            self._nbt = cnt
        if self._bnbuf is None:      # running statistics as views of one tensor: one broadcast per forward
            from .. import dist as cdist
            self._bnbuf = cdist.flatten_bn_buffers(self, device)
        return self

    def cuda(self, device=None):
        return self.setup(torch.device("cuda", device) if isinstance(device, int) else device)

    def to(self, *args, **kwargs):
        device = kwargs.get("device", args[0] if args else None)
        if isinstance(device, (str, torch.device)) and torch.device(device).type == "cuda":
            return self.setup(device)
        if self.store is not None:
            raise RuntimeError("parameters are flattened on the GPU; .to() other than cuda is not supported")
        return super().to(*args, **kwargs)

    def load_state_dict(self, state_dict, strict=True, assign=False):
        r = super().load_state_dict(state_dict, strict=strict)
        if self.store is not None:
            self.store.refresh_shadow()
        return r

    # ------------------------------------------------------------------ stochastic masks
    def _stochastic(self, B, device):
        """DropPath per-sample scales (n_blocks, 2 [attn, mlp], 2*B) and Dropout2d (B, E)."""
        if not self.training:
            return None, None
        key = (B, str(device))
        cache = self.__dict__.setdefault("_keep_cache", {})
        if key not in cache:   # built once: no host->device copy inside a captured graph
            keep = torch.tensor(self.backbone.drop_path_keep_probs(), dtype=torch.float32)  # (nb, 2 streams)
            cache[key] = keep[:, None, :, None].expand(-1, 2, -1, B).reshape(len(keep), 2, 2 * B).to(device)
        keep = cache[key]
        p = self.decode_head.dropout_ratio
        E = self.decode_head.embed_dim
        if self.forced_masks is not None:
            dp = self.forced_masks["droppath"].to(device=device, dtype=torch.float32)
            d2 = self.forced_masks.get("dropout2d")
            d2 = (d2.to(device=device, dtype=torch.float32) / (1 - p)).contiguous() if (p > 0 and d2 is not None) \
                else None
            return (dp / keep).contiguous(), d2
        # one launch draws both masks (counter-based RNG, step counter on the device, so graph
        # replays draw fresh masks) and bumps num_batches_tracked: cmx_step_masks
        st = self.__dict__.get("_mask_state")
        if st is None or st[1].device != keep.device:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())       # from torch's host generator
            st = self.__dict__["_mask_state"] = (seed, torch.zeros(1, dtype=torch.int64, device=device))
        dp = torch.empty_like(keep)
        d2 = torch.empty(B, E, device=device) if p > 0 else None
        nbt = getattr(self, "_nbt", None)
        K.call("cmx_step_masks", keep, keep.numel(), dp, B * E if d2 is not None else 0, float(p), d2, st[0], st[1], nbt,
               nbt.numel() if nbt is not None else 0)
        self._nbt_bumped = True
        return dp, d2

    # ------------------------------------------------------------------ forward
    def _logits_lowres(self, rgb, modal_x, with_aux=False):
        """(low-res logits, their grid, (aux logits, their grid) or None)."""
        if self.store is None:
            raise RuntimeError("call model.cuda() first: EncoderDecoder has no CPU execution path")
        B, _, H, W = rgb.shape
        dev = self.store.device
        if self.training and torch.is_grad_enabled() and not torch.cuda.is_current_stream_capturing():
            self.store.ensure_grads()
        rgb = rgb.to(device=dev, dtype=torch.float32).contiguous()
        modal_x = modal_x.to(device=dev, dtype=torch.float32).contiguous()
        images = (rgb, modal_x)            # the stage-1 im2col reads both batches (no concat)
        self._nbt_bumped = False
        pg = self.process_group
        if self.training and self.broadcast_buffers and pg is not None and self._bnbuf is not None:
            import torch.distributed as tdist
            if tdist.get_world_size(pg) > 1:
                from .. import dist as cdist
                cdist.broadcast_buffers(self._bnbuf, pg)
        dp, d2 = self._stochastic(B, dev)
        group = self.process_group if (self.sync_bn and self.training) else None
        if self.training and getattr(self, "_nbt", None) is not None and not self._nbt_bumped:
            self._nbt.add_(1)
        # forced_masks["aspp_dropout"] (optional): the (B, h, w, C4) 0/1 mask of the eASPP neck's Dropout; without
        # it the neck draws its mask on the device (eASPP.dropout_scale), inside a captured step too
        am = self.forced_masks.get("aspp_dropout") if (self.training and self.forced_masks is not None) else None
        feats, grids = self.backbone.run(self.store, images, B, H, W, self.training, dp, aspp_mask=am)
        head = self.decode_head
        if isinstance(head, FCNHead):      # one stage map; the logits live on that stage's grid
            i = head.out_index
            logits = head.run(self.store, feats[i], B, *grids[i], self.training, group=group)
        else:
            i = 0
            if isinstance(head, DeepLabV3Plus):     # its two elementwise Dropouts take their forced masks from here
                head.forced_masks = self.forced_masks if self.training else None
            logits = head.run(self.store, feats, grids, B, self.training, dscale=d2, group=group)
        aux = None
        if with_aux and self.aux_head is not None:
            j = self.aux_index
            aux = (self.aux_head.run(self.store, feats[j], B, *grids[j], self.training, group=group), grids[j])
        return logits, grids[i], aux

    def encode_decode(self, rgb, modal_x):
        # without a label the auxiliary head is not run: its result would be discarded (builder.py:240-253)
        logits, (h, w), _ = self._logits_lowres(rgb, modal_x)
        B, _, H, W = rgb.shape
        return F.upsample_logits_nchw(logits, B, h, w, H, W, self.num_classes)

    def _scaled_loss(self, logits, label, dims):
        return F.UpsampleScaledLossF.apply(logits, label, dims, self.ignore_index, self._loss_spec, self._loss_weight)

    def forward(self, rgb, modal_x, label=None):
        if label is None:
            return self.encode_decode(rgb, modal_x)
        logits, (h, w), aux = self._logits_lowres(rgb, modal_x, with_aux=True)
        B, _, H, W = rgb.shape
        label = label.to(device=logits.device, dtype=torch.int64).contiguous()
        dims = (B, h, w, H, W, self.num_classes)
        loss = self._main_loss(logits, label, dims)
        if aux is not None:
            # builder.py:250-251, in train and eval mode alike: + aux_rate * criterion(aux logits upsampled, label)
            alog, (ha, wa) = aux
            aux_loss = self._scaled_loss(alog, label, (B, ha, wa, H, W, self.num_classes))
            loss = torch.add(loss, aux_loss, alpha=self.aux_rate)      # one launch
        return loss

    def _main_loss(self, logits, label, dims):
        B, h, w, H, W, _ = dims
        if (H, W) != (4 * h, 4 * w) and isinstance(self.decode_head, FCNHead):
            return self._scaled_loss(logits, label, dims)
        if self._loss_spec is None:        # plain CrossEntropyLoss
            return F.UpsampleCEF.apply(logits, label, dims, self.ignore_index)
        if isinstance(self._loss_spec, DiceSpec):
            return F.UpsampleDiceF.apply(logits, label, dims, self.ignore_index, self._loss_spec)
        if isinstance(self._loss_spec, OhemSpec):
            return F.UpsampleOhemF.apply(logits, label, dims, self.ignore_index, self._loss_spec)
        return F.UpsampleLossF.apply(logits, label, dims, self.ignore_index, self._loss_spec, self._loss_weight)
