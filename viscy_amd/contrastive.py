"""DynaCLR contrastive path on MI355X: drop-ins for

  * ``viscy_models.contrastive.ContrastiveEncoder``  (/root/reference/packages/viscy-models/src/viscy_models/contrastive/encoder.py:52-154)
  * ``viscy_models.contrastive.loss.NTXentLoss`` / ``NTXentHCL``  (.../contrastive/loss.py:20-186)
  * ``torch.nn.TripletMarginLoss`` (p = 2, no swap), the default ``loss_function`` of the reference's module
  * both training branches of ``dynaclr.engine.ContrastiveModule``: triplet (its default) and NT-Xent
    (applications/dynaclr/src/dynaclr/engine.py:33-347)

The trunk is the same ConvNeXt kernel schedule as the UNeXt2 encoder (``viscy_amd.engine_unext2``: stem patch GEMM, depthwise
7x7, LayerNorm, fc1 / GELU / GRN / fc2 GEMMs, 2x2 downsampling GEMMs); behind it ``vsx_avgpool_rows_*``, the LayerNorm kernel,
two small fp32 GEMMs and ``vsx_bn1d_*`` produce ``(embedding, projection)``; ``vsx_ntxent_*`` / ``vsx_triplet_*`` are the
losses.  Same constructor
keywords and ``state_dict()`` keys as the reference (timm names: ``stem.conv``, ``encoder.stem.1``,
``encoder.stages.i.{downsample.{0,1},blocks.j.{[gamma,]conv_dw,norm,mlp.fc1,[mlp.grn,]mlp.fc2}}``, ``encoder.head.norm``,
``projection.{0,1,3,4}`` incl. the BatchNorm buffers), parameters shared with the flat-buffer engine so the fused AdamW and
the RCCL gradient all-reduce work unchanged.

Built: ``backbone="convnext_tiny"`` (V1 blocks: layer scale ``gamma`` folded into fc2 by ``vsx_layer_scale_fold`` /
``_unfold``, identity GRN) and ``"convnextv2_tiny"`` (GRN blocks); ``resnet50`` raises ``NotImplementedError``;
``pretrained`` must be False (no network here); ``drop_path_rate`` is timm's linear stochastic-depth schedule (training mode).  BatchNorm is per process
under data parallelism, as in the reference's default (no SyncBatchNorm in its recipes' trainer sections).

``auxiliary_heads`` (``viscy_amd.heads.ClassificationHead``, the ``OPS-*`` recipes' gene classifier) run on the anchor's
embedding in the training and validation steps: total = contrastive + sum of weight * head loss, the head's gradient of the
embedding goes back through the trunk with the projection's, the heads' parameters live in a flat buffer of their own that the
module's one optimiser updates with the encoder's (one step count, one schedule).  The captured step (``make_train_step``) is
for modules without heads.

Not built: ``TripletMarginLoss`` with ``swap=True``, ``p != 2`` or ``reduction="none"``; ``nn.CosineEmbeddingLoss``; the
negative-pair matrices that the reference's ``_log_metrics`` adds for NT-Xent; a replacement ``projection``; image / PCA
logging, ``freeze_backbone``.
"""

from __future__ import annotations

import math
from typing import Literal, Sequence

import torch
from torch import Tensor, nn

from . import _lib as L
from .flat import CoreProxy
from .unext2 import Conv, Core, Encoder, Holder, LN, Stem


class _BN(Holder):
    def __init__(self, c: int):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(c))
        self.bias = nn.Parameter(torch.zeros(c))
        self.register_buffer("running_mean", torch.zeros(c))
        self.register_buffer("running_var", torch.ones(c))
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))


class _Tail(Holder):
    def __init__(self, feat: int, embedding_dim: int, projection_dim: int):
        super().__init__()
        self.norm = LN(feat)
        self.fc0, self.bn1 = Conv((embedding_dim, feat)), _BN(embedding_dim)
        self.fc3, self.bn4 = Conv((projection_dim, embedding_dim)), _BN(projection_dim)


class _EmbedCore(Core):
    def __init__(self, in_channels, in_stack_depth, stem_kernel_size, depths, dims, embedding_dim, projection_dim, v1):
        super().__init__()
        kz = stem_kernel_size[0]
        ratio = (in_stack_depth - kz) // kz + 1
        mismatch = dims[0] - ratio * (dims[0] // ratio)
        if mismatch != 0:  # stems.py:113-119
            raise ValueError(f"Stem needs to output {mismatch} more channels to match the encoder. Adjust the in_stack_depth.")
        if in_stack_depth % kz:
            raise NotImplementedError("in_stack_depth must be a multiple of the stem kernel depth (stride == kernel)")
        self.cfg = dict(in_channels=in_channels, out_channels=0, in_stack_depth=in_stack_depth, out_stack_depth=0,
                        depths=tuple(depths), dims=tuple(dims), conv_mlp=False, stem_kernel=tuple(stem_kernel_size), ratio=ratio,
                        head="embed")
        self.encoder_stages = Encoder(depths, dims, False, v1=v1)
        self.stem = Stem(in_channels, dims[0] // ratio, tuple(stem_kernel_size))
        self.tail = _Tail(dims[-1], embedding_dim, projection_dim)
        self.reset_parameters()

    def reset_parameters(self) -> None:
        for name, mod in self.named_modules():
            if isinstance(mod, Conv) and name.startswith("encoder_stages"):  # timm _init_weights
                nn.init.trunc_normal_(mod.weight, std=0.02)
                nn.init.zeros_(mod.bias)
        for conv in (self.stem.conv, self.tail.fc0, self.tail.fc3):  # torch defaults (Conv3d / Linear)
            nn.init.kaiming_uniform_(conv.weight, a=math.sqrt(5))
            bound = 1 / math.sqrt(conv.weight[0].numel())
            nn.init.uniform_(conv.bias, -bound, bound)


class ContrastiveEncoder(CoreProxy, nn.Module):
    def __init__(self, backbone: Literal["convnext_tiny", "convnextv2_tiny", "resnet50"], in_channels: int, in_stack_depth: int,
                 stem_kernel_size: Sequence[int] = (5, 4, 4), stem_stride: Sequence[int] = (5, 4, 4), embedding_dim: int = 768,
                 projection_dim: int = 128, drop_path_rate: float = 0.0, pretrained: bool = False,
                 depths: Sequence[int] = (3, 3, 9, 3), dims: Sequence[int] = (96, 192, 384, 768)) -> None:
        """``depths`` / ``dims`` are an extension for tests (the reference takes them from the timm model name)."""
        super().__init__()
        if backbone not in ("convnext_tiny", "convnextv2_tiny"):
            raise NotImplementedError(f"backbone {backbone!r}: viscy_amd builds the convnext_tiny / convnextv2_tiny trunks")
        if pretrained:
            raise NotImplementedError("pretrained timm weights cannot be downloaded here; load a state_dict instead")
        if not 0.0 <= float(drop_path_rate) < 1.0:
            raise ValueError(f"drop_path_rate must be in [0, 1), got {drop_path_rate}")
        if tuple(stem_kernel_size) != tuple(stem_stride):
            raise NotImplementedError("stem_stride must equal stem_kernel_size (patchifying stem)")
        if embedding_dim % 4 or projection_dim % 4:
            raise NotImplementedError("embedding_dim and projection_dim must be multiples of 4")
        self.backbone = backbone
        core = _EmbedCore(in_channels, in_stack_depth, tuple(stem_kernel_size), tuple(depths), tuple(dims), embedding_dim, projection_dim,
                          v1=backbone == "convnext_tiny")
        if drop_path_rate:  # timm ConvNeXt: rates rise linearly over all blocks; active in training mode only
            core.cfg["drop_path"] = torch.linspace(0, float(drop_path_rate), sum(depths)).tolist()
        object.__setattr__(self, "_core", core)  # NOT a registered submodule: its parameters appear below, under reference names
        self.stem = core.stem
        enc = Holder()
        enc.stem = nn.Sequential(nn.Identity(), core.encoder_stages.stem_1)
        enc.stages = nn.Sequential(*[getattr(core.encoder_stages, f"stages_{i}") for i in range(4)])
        enc.norm_pre = nn.Identity()
        head = Holder()
        head.norm = core.tail.norm
        enc.head = head
        self.encoder = enc
        self.projection = nn.Sequential(core.tail.fc0, core.tail.bn1, nn.ReLU(inplace=True), core.tail.fc3, core.tail.bn4)

    def forward(self, x: Tensor) -> tuple[Tensor, Tensor]:
        """(embedding [B, num_features], projection [B, projection_dim]) — encoder.py:138-154"""
        return self._core(x)

    def forward_groups(self, x: Tensor, groups: int) -> tuple[Tensor, Tensor]:
        """``groups`` batches concatenated along dim 0, equal to ``groups`` separate ``forward`` calls (BatchNorm batch
        statistics and running-statistics updates per group, in order) with ONE pass of the trunk: half the launches and
        twice the rows per GEMM for the (anchor, positive) step"""
        return self._core(x, None, groups)


# ------------------------------------------------------------------------------------------------ losses
class _NTXentFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, embeddings: Tensor, labels: Tensor, temperature: float, beta: float):
        from . import ops as O

        acc, saved = O.ntxent_fwd(embeddings.contiguous().float(), labels.to(torch.int32).contiguous(), temperature, beta)
        ctx.saved, ctx.acc, ctx.in_dtype = saved, acc, embeddings.dtype
        return acc[0].clone()

    @staticmethod
    def backward(ctx, gout: Tensor):
        from . import ops as O

        return O.ntxent_bwd(ctx.saved, ctx.acc, gout.contiguous().float()).to(ctx.in_dtype), None, None, None


class _TripletFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, anchor: Tensor, positive: Tensor, negative: Tensor, margin: float, eps: float, reduction: str):
        from . import ops as O

        a, p_, n = (t.contiguous().float() for t in (anchor, positive, negative))
        rows, acc = O.triplet_fwd(a, p_, n, margin, eps, reduction)
        ctx.save_for_backward(a, p_, n, rows)
        ctx.args, ctx.in_dtypes = (margin, eps, reduction), (anchor.dtype, positive.dtype, negative.dtype)
        ctx.mark_non_differentiable(acc)
        return acc[0].clone(), acc

    @staticmethod
    def backward(ctx, gout: Tensor, _gacc):
        from . import ops as O

        a, p_, n, rows = ctx.saved_tensors
        grads = O.triplet_bwd(a, p_, n, rows, gout.contiguous().float(), *ctx.args)
        return (*(g.to(dt) for g, dt in zip(grads, ctx.in_dtypes)), None, None, None)


def cosine_anneal(start: float, end: float, epoch: int, warmup_epochs: int) -> float:
    """viscy_models/schedule.py:8-33"""
    if epoch >= warmup_epochs:
        return end
    return end + (start - end) * 0.5 * (1.0 + math.cos(math.pi * epoch / warmup_epochs))


class NTXentLoss(nn.Module):
    """NT-Xent over cosine similarities with an optional temperature schedule (loss.py:20-73): ``loss(embeddings, labels)``,
    every ordered pair of distinct samples with equal labels is a positive pair, all samples with another label are its
    negatives, mean over positive pairs."""

    beta = 0.0

    def __init__(self, temperature: float = 0.07, temperature_schedule: Literal["cosine", "constant"] = "constant",
                 temperature_start: float = 0.1, temperature_warmup_epochs: int = 50, **kwargs):
        super().__init__()
        if kwargs:
            raise NotImplementedError(f"pytorch-metric-learning options {sorted(kwargs)} are not built")
        self.temperature = temperature
        self.temperature_schedule, self.temperature_start = temperature_schedule, temperature_start
        self.temperature_end, self.temperature_warmup_epochs = temperature, temperature_warmup_epochs

    def step(self, epoch: int) -> None:
        if self.temperature_schedule == "cosine":
            self.temperature = cosine_anneal(self.temperature_start, self.temperature_end, epoch, self.temperature_warmup_epochs)

    def forward(self, embeddings: Tensor, labels: Tensor) -> Tensor:
        if not embeddings.is_cuda:
            raise RuntimeError(f"viscy_amd.{type(self).__name__} runs on MI355X HIP kernels only (no CPU / eager fallback)")
        if embeddings.ndim != 2 or labels.shape != embeddings.shape[:1]:
            raise ValueError(f"embeddings must be (N, D) and labels (N,), got {tuple(embeddings.shape)} / {tuple(labels.shape)}")
        L.lib()
        return _NTXentFn.apply(embeddings, labels, float(self.temperature), float(self.beta))


class NTXentHCL(NTXentLoss):
    """hard-negative concentration (loss.py:76-186): each negative's term in the denominator is weighted by
    ``exp(beta * sim)``, weights normalised to sum to the number of negatives; ``beta = 0`` is plain NT-Xent."""

    def __init__(self, temperature: float = 0.07, beta: float = 0.5, **kwargs):
        super().__init__(temperature=temperature, **kwargs)
        self.beta = beta


class TripletMarginLoss(nn.Module):
    """``torch.nn.TripletMarginLoss`` with its keywords and defaults: ``loss(anchor, positive, negative)`` on ``(B, D)``
    tensors, mean or sum over rows of ``max(d(a, p) - d(a, n) + margin, 0)`` with ``d = F.pairwise_distance``.  Built: ``p = 2``,
    ``swap=False``, ``reduction`` "mean" / "sum".  After a forward ``last_stats`` holds, detached, the six numbers that
    ``vsx_triplet_fwd`` sums in a fixed order: {loss, mean cosine similarity (a, p), mean distance (a, p), mean cosine
    similarity (a, n), mean distance (a, n), share of rows with a positive hinge}."""

    def __init__(self, margin: float = 1.0, p: float = 2.0, eps: float = 1e-6, swap: bool = False, reduction: str = "mean"):
        super().__init__()
        if float(p) != 2.0:
            raise NotImplementedError(f"TripletMarginLoss p={p}: viscy_amd builds the Euclidean distance (p=2)")
        if swap:
            raise NotImplementedError("TripletMarginLoss swap=True (distance swap) is not built")
        if reduction == "none":
            raise NotImplementedError('TripletMarginLoss reduction="none" is not built ("mean" / "sum")')
        if reduction not in ("mean", "sum"):
            raise ValueError(f"{reduction} is not a valid value for reduction")
        self.margin, self.p, self.eps, self.swap, self.reduction = float(margin), 2.0, float(eps), False, reduction
        self.last_stats: Tensor | None = None

    @classmethod
    def from_torch(cls, loss: nn.TripletMarginLoss) -> "TripletMarginLoss":
        return cls(margin=loss.margin, p=loss.p, eps=loss.eps, swap=loss.swap, reduction=loss.reduction)

    def forward(self, anchor: Tensor, positive: Tensor, negative: Tensor) -> Tensor:
        if anchor.ndim != 2 or positive.shape != anchor.shape or negative.shape != anchor.shape or anchor.numel() == 0:
            raise ValueError("anchor, positive and negative must be non-empty (B, D) tensors of equal shape, got "
                             f"{tuple(anchor.shape)} / {tuple(positive.shape)} / {tuple(negative.shape)}")
        if not (anchor.is_cuda and positive.is_cuda and negative.is_cuda):
            raise RuntimeError(f"viscy_amd.{type(self).__name__} runs on MI355X HIP kernels only (no CPU / eager fallback)")
        L.lib()
        loss, acc = _TripletFn.apply(anchor, positive, negative, self.margin, self.eps, self.reduction)
        self.last_stats = acc.detach()
        return loss


# ------------------------------------------------------------------------------------------------ engine
class ContrastiveModule(nn.Module):
    """``dynaclr.engine.ContrastiveModule`` (engine.py:33-347): ``training_step`` / ``validation_step`` on a ``TripletSample``
    (``anchor``, ``positive`` and, for the triplet branch, ``negative``), ``predict_step`` -> features / projections,
    ``on_train_epoch_start`` temperature schedule, ``configure_optimizers`` -> fused flat AdamW.  ``loss_function``: the
    NT-Xent family (the default here) or ``TripletMarginLoss`` (the reference's default; a ``torch.nn.TripletMarginLoss``
    instance is converted), ``auxiliary_heads``: ``{name: viscy_amd.heads.ClassificationHead}``.  The cosine-embedding loss, a
    replacement ``projection`` and image / PCA logging are not built."""

    def __init__(self, encoder: ContrastiveEncoder, loss_function: nn.Module | None = None, lr: float = 1e-3,
                 schedule: Literal["WarmupCosine", "Constant"] = "Constant", log_batches_per_epoch: int = 8,
                 log_samples_per_batch: int = 1, example_input_array_shape: Sequence[int] = (1, 2, 15, 256, 256),
                 ckpt_path: str | None = None, freeze_backbone: bool = False, gather_embeddings: bool = False,
                 projection: nn.Module | None = None, auxiliary_heads: dict | None = None, **unused) -> None:
        super().__init__()
        if freeze_backbone:
            raise NotImplementedError("freeze_backbone is not built (the fused flat-buffer optimiser updates every parameter)")
        if projection is not None:
            raise NotImplementedError("projection: replacing the encoder's projection MLP is not built (the embedding tail is "
                                      "part of the encoder's kernel schedule)")
        self.model = encoder
        from .heads import BaseHead, ClassificationHead

        for name, head in (auxiliary_heads or {}).items():
            if not isinstance(head, BaseHead):
                raise TypeError(f"auxiliary_heads[{name!r}] must be a viscy_amd.heads.BaseHead, got {type(head).__name__}")
            if not isinstance(head, ClassificationHead):
                raise NotImplementedError(f"auxiliary_heads[{name!r}]: {type(head).__name__} is not built (ClassificationHead is)")
        self.auxiliary_heads = nn.ModuleDict(auxiliary_heads or {})
        self._heads_engine = None
        if isinstance(loss_function, nn.TripletMarginLoss):  # the reference's default / YAML class_path
            loss_function = TripletMarginLoss.from_torch(loss_function)
        self.loss_function = loss_function if loss_function is not None else NTXentLoss()
        if isinstance(self.loss_function, nn.CosineEmbeddingLoss):
            raise NotImplementedError("CosineEmbeddingLoss is not built: the reference's non-NT-Xent branch calls loss(anchor, "
                                      "positive, negative), which hands the negative projection to it as its `target`")
        if not isinstance(self.loss_function, (NTXentLoss, TripletMarginLoss)):
            raise NotImplementedError(f"{type(self.loss_function).__name__}: viscy_amd builds the NT-Xent family and "
                                      "TripletMarginLoss of the DynaCLR losses")
        self.triplet = isinstance(self.loss_function, TripletMarginLoss)
        if self.triplet and gather_embeddings:
            raise NotImplementedError("gather_embeddings widens the NT-Xent negatives; a triplet row has its own negative")
        self.lr, self.schedule = lr, schedule
        self.log_batches_per_epoch, self.log_samples_per_batch = log_batches_per_epoch, log_samples_per_batch
        self.example_input_array = torch.rand(*example_input_array_shape)
        # extension beyond the reference (BASELINE config 5): under torch.distributed the projections of all ranks are
        # all-gathered so that every anchor sees world * 2B - 2 negatives instead of 2B - 2; False = the reference's behaviour
        self.gather_embeddings = gather_embeddings
        self.paired_forward = True  # False: separate forwards per view, literally as the reference does
        self.current_epoch = 0
        self._logging = True
        self.logged: dict[str, list] = {}
        if ckpt_path is not None:
            self.load_state_dict(torch.load(ckpt_path, weights_only=True, map_location="cpu")["state_dict"], strict=False)

    def _log(self, key: str, value) -> None:
        if self._logging:
            self.logged.setdefault(key, []).append(value.detach() if torch.is_tensor(value) else value)

    def make_train_step(self, optimizer, ddp=None, use_graph: bool = True):
        """the whole contrastive step (zero-grad, the forwards, the loss, backward, fused AdamW) as ONE hipGraph replay per batch
        (``viscy_amd.step.TrainStep``); call ``step(anchor, positive) -> loss`` with fixed shapes, or, with a triplet loss,
        ``step(anchor, positive, negative) -> loss``"""
        from .step import TrainStep

        if len(self.auxiliary_heads):
            raise NotImplementedError("auxiliary heads run on the eager step (training_step / Trainer.fit): the captured step "
                                      "carries (anchor, positive[, negative]) and no labels")

        def loss_fn(anchor, other):
            batch = {"anchor": anchor, "positive": other}
            if self.triplet:  # TrainStep carries two tensors: (positive, negative) travel stacked
                batch = {"anchor": anchor, "positive": other[0], "negative": other[1]}
            was, self._logging = self._logging, False  # the captured tensors must not pile up in the log
            try:
                return self._step(batch, "train")
            finally:
                self._logging = was

        step = TrainStep(self.model, None, optimizer, ddp=ddp, use_graph=use_graph, loss_fn=loss_fn)
        if self.triplet:
            return lambda anchor, positive, negative: step(anchor, torch.stack((positive, negative)))
        return step

    def on_train_epoch_start(self) -> None:
        if hasattr(self.loss_function, "step"):
            self.loss_function.step(self.current_epoch)
        if hasattr(self.loss_function, "temperature"):
            self._log("hparams/temperature", self.loss_function.temperature)
        for head in self.auxiliary_heads.values():
            head.step(self.current_epoch)
            self._log(f"hparams/loss_weight/{head.head_name}", head.get_weight())

    # ------------------------------------------------------------------ auxiliary heads (engine.py:227-260)
    def heads_engine(self, ops=None):
        """the ``AuxHeadsEngine`` over all heads of this module (one flat fp32 parameter / gradient buffer); None without heads"""
        heads = list(self.auxiliary_heads.values())
        if not heads:
            return None
        from .heads import AuxHeadsEngine

        eng = self._heads_engine
        dev = next(self.auxiliary_heads.parameters()).device
        if eng is None or eng.device != dev or (ops is not None and eng.ops is not ops) or any(h._engine is not eng for h in heads):
            eng = self._heads_engine = AuxHeadsEngine(self.auxiliary_heads, ops)
        return eng

    def _get_labels(self, batch: dict, batch_key: str) -> Tensor | None:
        """a top-level batch key first, then ``anchor_meta[i]["labels"][batch_key]`` as a long tensor; None where neither has it"""
        if batch_key in batch:
            y = batch[batch_key]
        else:
            meta = batch.get("anchor_meta")
            if not meta or "labels" not in meta[0] or batch_key not in meta[0]["labels"]:
                return None
            vals = [m["labels"][batch_key] for m in meta]
            if isinstance(vals[0], (list, tuple)) or getattr(vals[0], "ndim", 0) > 0:   # the reference stacks these as floats
                raise NotImplementedError(f"vector-valued labels ({batch_key!r}) belong to CrossModalContrastiveHead, which is not built")
            y = torch.tensor([int(v) for v in vals], dtype=torch.long, device=batch["anchor"].device)
        if not torch.is_tensor(y) or y.ndim != 1 or y.is_floating_point():
            raise NotImplementedError(f"vector-valued labels ({batch_key!r}) belong to CrossModalContrastiveHead, which is not built")
        return y

    def _run_auxiliary_heads(self, anchor_features: Tensor, batch: dict, stage: str) -> Tensor | None:
        """sum of weight * loss over the heads whose labels the batch carries (None if there is none), logging each head's
        loss and accuracies"""
        aux = None
        if len(self.auxiliary_heads):
            self.heads_engine()
        for head in self.auxiliary_heads.values():
            y = self._get_labels(batch, head.batch_key)
            if y is None:
                continue
            head_loss, stats = head.loss_and_stats(anchor_features, y)
            term = head.get_weight() * head_loss
            aux = term if aux is None else aux + term
            if self._logging:
                head.log_metrics({"loss": head_loss, "stats": stats}, self._log, stage)
        return aux

    def forward(self, x: Tensor) -> tuple[Tensor, Tensor]:
        return self.model(x)

    def _step_triplet(self, batch: dict, stage: str) -> Tensor:
        if "negative" not in batch:
            raise KeyError("negative: the triplet branch needs batch['negative'] next to 'anchor' and 'positive'")
        views = (batch["anchor"], batch["positive"], batch["negative"])
        if self.paired_forward and views[0].shape == views[1].shape == views[2].shape:
            # one trunk pass over [anchor; positive; negative]; BatchNorm statistics and running-statistics updates per view,
            # in this order, as the reference's three calls make them (dynaclr/engine.py:265-266,276)
            emb, proj = self.model.forward_groups(torch.cat(views), 3)
            projections, anchor_features = proj.chunk(3), emb[: views[0].shape[0]]
        else:
            outs = tuple(self(v) for v in views)
            projections, anchor_features = tuple(o[1] for o in outs), outs[0][0]
        loss = self.loss_function(*projections)
        self._log(f"loss/{stage}", loss)
        if self._logging:  # engine.py:135-146, from the sums the loss kernels formed anyway
            st = self.loss_function.last_stats
            self._log(f"metrics/cosine_similarity/positive/{stage}", st[1])
            self._log(f"metrics/euclidean_distance/positive/{stage}", st[2])
            self._log(f"metrics/cosine_similarity_negative/{stage}", st[3])
            self._log(f"metrics/euclidean_distance_negative/{stage}", st[4])
        aux = self._run_auxiliary_heads(anchor_features, batch, stage)
        return loss if aux is None else loss + aux

    def _step(self, batch: dict, stage: str) -> Tensor:
        if self.triplet:
            return self._step_triplet(batch, stage)
        a, p_ = batch["anchor"], batch["positive"]
        if self.paired_forward and a.shape == p_.shape:
            # one trunk pass over [anchor; positive]; BatchNorm statistics stay per call (dynaclr/engine.py:265-266)
            emb, proj = self.model.forward_groups(torch.cat((a, p_)), 2)
            anchor_projection, positive_projection = proj[: a.shape[0]], proj[a.shape[0]:]
            anchor_features = emb[: a.shape[0]]
        else:
            anchor_features, anchor_projection = self(a)
            _, positive_projection = self(p_)
        if self.gather_embeddings:
            from .parallel import all_gather_with_local_grad, scale_for_mean_reduction

            anchor_projection = all_gather_with_local_grad(anchor_projection)
            positive_projection = all_gather_with_local_grad(positive_projection)
        indices = torch.arange(0, anchor_projection.size(0), device=anchor_projection.device)
        loss = self.loss_function(torch.cat((anchor_projection, positive_projection)), torch.cat((indices, indices)))
        self._log(f"loss/{stage}", loss)
        if self.gather_embeddings:
            loss = scale_for_mean_reduction(loss)
        aux = self._run_auxiliary_heads(anchor_features, batch, stage)  # a mean over the local batch already: added unscaled
        return loss if aux is None else loss + aux

    def training_step(self, batch: dict, batch_idx: int) -> Tensor:
        return self._step(batch, "train")

    def validation_step(self, batch: dict, batch_idx: int, dataloader_idx: int = 0) -> Tensor:
        return self._step(batch, "val")

    def predict_step(self, batch: dict, batch_idx: int, dataloader_idx: int = 0) -> dict:
        features, projections = self.model(batch["anchor"])
        return {"features": features, "projections": projections, "index": batch.get("index")}

    def configure_optimizers(self, t_total: int | None = None):
        from .optim import FlatAdamW

        self.model.grad_mode = "flat"
        heads = self.heads_engine()
        if heads is None:
            return FlatAdamW(self.model.engine(), lr=self.lr, schedule=self.schedule, t_total=t_total or 0)
        from .optim import MultiFlatAdamW

        for head in self.auxiliary_heads.values():
            head.grad_mode = "flat"
        # AdamW(self.parameters(), lr) of the reference: one step count and one schedule over the encoder's and the heads' buffers
        return MultiFlatAdamW(self.model.engine(), [heads], lr=self.lr, schedule=self.schedule, t_total=t_total or 0)
