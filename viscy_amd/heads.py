"""Embedding-space task heads of the DynaCLR recipes on MI355X: drop-ins for ``viscy_models.components.heads``

  * ``BaseHead``            (heads.py:34-156)   name, batch key and the (optionally cosine-annealed) loss weight
  * ``ClassificationHead``  (heads.py:159-272)  ``MLP`` in classification mode + cross-entropy + top-1 / top-k accuracy
  * ``CosineClassifier``    (heads.py:420-453)  L2-normalised linear classifier with a learnable log temperature
  * ``MLP``                 (heads.py:456-591)  classification mode: (Linear -> BatchNorm1d -> ReLU) x n -> classifier

Same constructor keywords, defaults, initialisation and ``state_dict()`` keys as the reference (``mlp.backbone.{3i}`` Linear,
``mlp.backbone.{3i+1}`` BatchNorm1d incl. its buffers, ``mlp.head.{weight, log_scale | bias}``).  The hidden layers run on the
fp32 GEMMs and ``vsx_bn1d_*``; the classifier and its loss are ``vsx_cls_ce_*`` (csrc/aux_head.hip), which never store the
[B, C] logits on the training path.  Training therefore enters through ONE fused call,

    loss, stats = head.loss_and_stats(features, labels)     # stats: top1, topk, n_valid as device tensors

differentiable with respect to ``features`` and the head's parameters; ``forward(x)`` materialises logits for inference and
refuses an input that requires grad, ``compute_loss(logits, y)`` points to the fused entry.

The parameters of all heads of a module live in one flat fp32 buffer of their own (``AuxHeadsEngine``, a ``FlatEngine`` that
takes an ``ops`` backend like the others); the encoder's flat layout, a checkpoint format, is untouched.

Not built (each raises ``NotImplementedError`` naming itself): ``MLP`` in projection mode, ``norm="ln"``, ``dropout > 0``,
activations other than ReLU, ``CrossModalContrastiveHead``; widths that are not multiples of 4.
"""

from __future__ import annotations

import math
from typing import Literal

import torch
from torch import Tensor, nn

from . import _lib as L
from . import ops as hip_ops
from .flat import FlatEngine


def _holder_forward(self, *a, **k):  # pragma: no cover
    raise RuntimeError("viscy_amd parameter holder: run the head through ClassificationHead.loss_and_stats / forward (HIP kernels)")


class _Linear(nn.Linear):
    """torch's parameters and initialisation; never called"""

    forward = _holder_forward


class _BatchNorm1d(nn.BatchNorm1d):
    forward = _holder_forward


class _ReLU(nn.ReLU):
    forward = _holder_forward


class CosineClassifier(nn.Module):
    """``exp(log_scale) * normalize(x) @ normalize(weight).T`` (heads.py:420-453); parameter holder"""

    def __init__(self, in_dim: int, num_classes: int, init_scale: float = 20.0, learn_scale: bool = True):
        super().__init__()
        self.weight = nn.Parameter(torch.randn(num_classes, in_dim))
        nn.init.normal_(self.weight, std=0.01)
        if learn_scale:
            self.log_scale = nn.Parameter(torch.tensor(math.log(init_scale)))
        else:
            self.register_buffer("log_scale", torch.tensor(math.log(init_scale)))

    forward = _holder_forward


class MLP(nn.Module):
    """``viscy_models.components.heads.MLP`` in classification mode (``num_classes`` set); parameter holder"""

    def __init__(self, in_dims: int, hidden_dims: int | list[int], out_dims: int | None = None, norm: Literal["bn", "ln"] = "bn",
                 activation: Literal["relu", "gelu", "silu"] = "relu", dropout: float = 0.0, num_classes: int | None = None,
                 cosine_classifier: bool = True) -> None:
        if num_classes is None and out_dims is None:
            raise ValueError("out_dims is required in projection mode (num_classes=None).")
        if num_classes is None:
            raise NotImplementedError("MLP projection mode (num_classes=None) is not built: viscy_amd builds the classification mode")
        if norm not in ("bn", "ln"):
            raise ValueError(f"norm must be 'bn' or 'ln', got '{norm}'")
        if norm != "bn":
            raise NotImplementedError("MLP norm='ln' is not built (BatchNorm1d hidden layers only)")
        if activation not in ("relu", "gelu", "silu"):
            raise ValueError(f"activation must be 'relu', 'gelu', or 'silu', got '{activation}'")
        if activation != "relu":
            raise NotImplementedError(f"MLP activation={activation!r} is not built (ReLU only)")
        if dropout > 0.0:
            raise NotImplementedError(f"MLP dropout={dropout} is not built (dropout > 0)")
        hidden_list = [hidden_dims] if isinstance(hidden_dims, int) else list(hidden_dims)
        if in_dims % 4 or any(h % 4 for h in hidden_list):
            raise NotImplementedError(f"MLP in_dims={in_dims}, hidden_dims={hidden_list}: widths must be multiples of 4 "
                                      "(rows of the fp32 GEMM)")
        if int(num_classes) < 1:
            raise ValueError(f"num_classes must be positive, got {num_classes}")
        super().__init__()
        self.input_dim = in_dims
        layers: list[nn.Module] = []
        prev = in_dims
        for h in hidden_list:
            layers += [_Linear(prev, h), _BatchNorm1d(h), _ReLU(inplace=True)]
            prev = h
        self.backbone = nn.Sequential(*layers)
        self.head: nn.Module = CosineClassifier(prev, num_classes) if cosine_classifier else _Linear(prev, num_classes)
        self.cosine, self.num_classes = bool(cosine_classifier), int(num_classes)

    def hidden(self):
        """[(Linear, BatchNorm1d), ...] in forward order"""
        mods = list(self.backbone)
        return [(mods[i], mods[i + 1]) for i in range(0, len(mods), 3)]

    forward = _holder_forward


# ------------------------------------------------------------------------------------------------ the flat-buffer engine
class AuxHeadsEngine(FlatEngine):
    """flat fp32 parameter / gradient buffers over the heads of one module, and each head's schedule: hidden layers on the
    fp32 GEMM + ``bn1d``, classifier + loss on ``cls_ce_*``.  ``model`` is the ``nn.ModuleDict`` (or any module) holding the
    heads; parameters are laid out head by head, each in backward order (classifier first), as ONE gradient bucket."""

    name = "ClassificationHead"

    def __init__(self, model, ops=None):
        ops = hip_ops if ops is None else ops
        self._hip = ops is hip_ops
        self._bucket_marks = [0]
        super().__init__(model, ops)
        for head in self.heads():
            head._engine = self

    def heads(self):
        return [m for m in self.model.modules() if isinstance(m, ClassificationHead)]

    def _param_order(self):
        ps = []
        for head in self.heads():
            mlp = head.mlp
            ps += [p for p in mlp.head.parameters()]
            for lin, bn in reversed(mlp.hidden()):
                ps += [bn.weight, bn.bias, lin.weight, lin.bias]
        self._bucket_marks.append(len(ps))
        return ps

    # ------------------------------------------------------------------ one head
    def _hidden_fwd(self, head, x: Tensor, saved: list | None):
        o = self.ops
        training = bool(head.training)
        h = x
        for lin, bn in head.mlp.hidden():
            n_out, n_in = lin.weight.shape
            B = h.shape[0]
            Wp, _ = o.prep_weight(lin.weight, n_out, n_in, 1, torch.float32, want=True, want_t=False)
            z = torch.empty((B, n_out), dtype=torch.float32, device=h.device)
            o.gemm("nt", h, Wp, z, B, n_out, n_in, n_in, n_in, n_out, dtype=torch.float32, epi=L.EPI_BIAS, bias=lin.bias)
            y, sm, sr = o.bn1d_fwd(z, bn.weight, bn.bias, bn.running_mean, bn.running_var, training, True)
            if training:
                bn.num_batches_tracked += 1
            if saved is not None:
                saved.append((h, z, y, sm, sr))
            h = y
        return h

    def _classifier(self, head, h: Tensor) -> dict:
        o, c = self.ops, head.mlp.head
        if head.mlp.cosine:
            return dict(inv_h=o.cls_inv_norm(h), inv_w=o.cls_inv_norm(c.weight), log_scale=c.log_scale.detach().view(1))
        return dict(bias=c.bias)

    def head_forward(self, head, x: Tensor, y: Tensor, need_bwd: bool):
        """-> (acc [4] = {loss, top-1, top-k, n_valid}, saved)"""
        saved = [] if need_bwd else None
        h = self._hidden_fwd(head, x, saved)
        cls = self._classifier(head, h)
        rows, acc = self.ops.cls_ce_fwd(h, head.mlp.head.weight, y, head.top_k, **cls)
        return acc, ((saved, h, y, cls, rows, acc, bool(head.training)) if need_bwd else None)

    def head_logits(self, head, x: Tensor) -> Tensor:
        h = self._hidden_fwd(head, x, None)
        return self.ops.cls_logits(h, head.mlp.head.weight, **self._classifier(head, h))

    def head_backward(self, head, sv, gout: Tensor) -> Tensor:
        """accumulates the head's parameter gradients into the flat gradient buffer; returns d loss / d x"""
        o, g = self.ops, self.g
        saved, h, y, cls, rows, acc, training = sv
        c = head.mlp.head
        if head.mlp.cosine:
            grads = dict(dlog_scale=g(c.log_scale).view(1)) if isinstance(c.log_scale, nn.Parameter) else dict(
                dlog_scale=o.zeros(1, device=h.device))
        else:
            grads = dict(dbias=g(c.bias))
        d = o.cls_ce_bwd(h, c.weight, y, rows, acc, gout, g(c.weight), **cls, **grads)
        for (lin, bn), (hin, z, yv, sm, sr) in zip(reversed(head.mlp.hidden()), reversed(saved)):
            n_out, n_in = lin.weight.shape
            B = hin.shape[0]
            dz = o.bn1d_bwd(d, z, yv, bn.weight, sm, sr, g(bn.weight), g(bn.bias), training, True)
            o.gemm("tn", hin, dz, g(lin.weight), B, n_out, n_in, n_in, n_out, n_in, dtype=torch.float32, colsum=g(lin.bias))
            _, WT = o.prep_weight(lin.weight, n_out, n_in, 1, torch.float32, want=False, want_t=True)
            d = torch.empty((B, n_in), dtype=torch.float32, device=hin.device)
            o.gemm("nt", dz, WT, d, B, n_in, n_out, n_out, n_out, n_in, dtype=torch.float32)
        return d

    def head_backward_autograd(self, head, sv, gout: Tensor):
        """autograd mode: ``head_backward`` into a zeroed buffer of its own -> (dx, one gradient per parameter of the head, in
        ``head.parameters()`` order); the flat gradient buffer is left as it was"""
        keep = self.flat_grad, self.grad_of
        try:
            self.flat_grad = self.ops.zeros(keep[0].numel(), device=keep[0].device)
            self.grad_of = self._grad_map(self.flat_grad)
            dx = self.head_backward(head, sv, gout)
            return dx, tuple(self.grad_of[id(p)] if p.requires_grad else None for p in head.parameters())
        finally:
            self.flat_grad, self.grad_of = keep


class _HeadLossFn(torch.autograd.Function):
    """one head as one autograd node: (x, y, head, need_bwd, *head.parameters()) -> (loss, acc)"""

    @staticmethod
    def forward(ctx, x, y, head, need_bwd, *params):
        acc, sv = head.engine().head_forward(head, x, y, need_bwd)
        ctx.head, ctx.sv, ctx.n = head, sv, len(params)
        ctx.mark_non_differentiable(acc)
        return acc[0].clone(), acc

    @staticmethod
    def backward(ctx, gout, _gacc):
        head, sv = ctx.head, ctx.sv
        if sv is None:
            raise RuntimeError("viscy_amd.ClassificationHead: backward called but the forward ran without gradient bookkeeping")
        ctx.sv = None
        eng = head.engine()
        gout = gout.contiguous().float().view(1)
        if head.grad_mode == "flat":
            return (eng.head_backward(head, sv, gout), None, None, None) + (None,) * ctx.n
        dx, grads = eng.head_backward_autograd(head, sv, gout)
        return (dx, None, None, None) + grads


# ------------------------------------------------------------------------------------------------ the public classes
class BaseHead(nn.Module):
    """``viscy_models.components.heads.BaseHead``: a pluggable task head that knows its batch key and its (scheduled) loss
    weight.  ``step(epoch)`` at the start of an epoch, ``get_weight()`` for the current weight."""

    def __init__(self, head_name: str, batch_key: str, loss_weight: float = 1.0,
                 weight_schedule: Literal["cosine", "constant"] = "constant", weight_start: float = 0.0,
                 weight_warmup_epochs: int = 50) -> None:
        super().__init__()
        self.head_name, self.batch_key = head_name, batch_key
        self.loss_weight, self.weight_schedule = loss_weight, weight_schedule
        self.weight_start, self.weight_warmup_epochs = weight_start, weight_warmup_epochs
        self._current_weight = weight_start if weight_schedule == "cosine" else loss_weight

    def step(self, epoch: int) -> None:
        if self.weight_schedule == "cosine":
            from .contrastive import cosine_anneal

            self._current_weight = cosine_anneal(self.weight_start, self.loss_weight, epoch, self.weight_warmup_epochs)

    def get_weight(self) -> float:
        return self._current_weight

    def forward(self, x: Tensor) -> Tensor:
        raise NotImplementedError

    def compute_loss(self, y_hat: Tensor, y: Tensor) -> Tensor:
        raise NotImplementedError

    def log_metrics(self, out: dict, log_fn, stage: str) -> None:
        raise NotImplementedError


class ClassificationHead(BaseHead):
    """``viscy_models.components.heads.ClassificationHead``: classification ``MLP`` + cross-entropy with top-1 / top-k
    accuracy.  Train through ``loss_and_stats(x, y)``; ``forward(x)`` gives materialised logits for inference."""

    grad_mode = "autograd"  # or "flat": gradients are written straight into the engine's flat gradient buffer
    _engine = None

    def __init__(self, head_name: str, batch_key: str, in_dims: int, hidden_dims: int | list[int], num_classes: int,
                 cosine_classifier: bool = True, loss_weight: float = 1.0, top_k: int = 5,
                 weight_schedule: Literal["cosine", "constant"] = "constant", weight_start: float = 0.0,
                 weight_warmup_epochs: int = 50) -> None:
        super().__init__(head_name=head_name, batch_key=batch_key, loss_weight=loss_weight, weight_schedule=weight_schedule,
                         weight_start=weight_start, weight_warmup_epochs=weight_warmup_epochs)
        if not 1 <= int(top_k) <= int(num_classes):  # logits.topk(top_k) raises there
            raise ValueError(f"top_k={top_k} must be in [1, num_classes={num_classes}]")
        self.mlp = MLP(in_dims=in_dims, hidden_dims=hidden_dims, num_classes=num_classes, cosine_classifier=cosine_classifier)
        self.top_k = int(top_k)

    # ------------------------------------------------------------------ engine plumbing
    def engine(self, ops=None) -> AuxHeadsEngine:
        """the ``AuxHeadsEngine`` that holds this head's parameters: the owning module's, or one of its own"""
        dev = next(self.parameters()).device
        eng = self._engine
        if eng is None or eng.device != dev or (ops is not None and eng.ops is not ops):
            eng = AuxHeadsEngine(self, ops)  # sets self._engine
        return eng

    def _apply(self, fn, *a, **k):
        self._engine = None  # parameter storage moves: flat views must be rebuilt
        return super()._apply(fn, *a, **k)

    def _check(self, x: Tensor) -> Tensor:
        if x.ndim != 2 or x.shape[1] != self.mlp.input_dim or x.shape[0] == 0:
            raise ValueError(f"features must be a non-empty (B, {self.mlp.input_dim}) tensor, got {tuple(x.shape)}")
        if self.engine()._hip:
            if not x.is_cuda:
                raise RuntimeError(f"viscy_amd.{type(self).__name__} runs on MI355X HIP kernels only (no CPU / eager fallback)")
            L.lib()
        return x

    # ------------------------------------------------------------------ the reference's surface
    def forward(self, x: Tensor) -> Tensor:
        """logits (B, num_classes), materialised: inference and inspection.  No gradient flows through this call."""
        if torch.is_grad_enabled() and x.requires_grad:
            raise RuntimeError("viscy_amd.ClassificationHead.forward materialises logits without an autograd history: the gradient "
                               "of the input would be lost; train through loss_and_stats(x, y)")
        self._check(x)
        with torch.no_grad():
            return self.engine().head_logits(self, x.detach().contiguous().float())

    def loss_and_stats(self, x: Tensor, y: Tensor) -> tuple[Tensor, dict[str, Tensor]]:
        """cross-entropy of the head's logits on ``x`` (B, in_dims) against integer labels ``y`` (B,) (``-100`` = ignored), and
        {"top1", "topk", "n_valid"} as detached device tensors; differentiable w.r.t. ``x`` and the head's parameters"""
        if x.ndim == 2 and (y.ndim != 1 or y.shape[0] != x.shape[0] or y.is_floating_point()):
            raise ValueError(f"labels must be {x.shape[0]} integer class indices, got {y.dtype} {tuple(y.shape)}")
        self._check(x)
        eng = self.engine()
        if self.grad_mode == "flat":
            eng.attach_grads()
        params = tuple(self.parameters())
        need_bwd = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params))
        with torch.autocast("cuda", enabled=False):
            loss, acc = _HeadLossFn.apply(x.contiguous().float(), y.to(device=x.device, dtype=torch.int64).contiguous(), self,
                                          need_bwd, *params)
        acc = acc.detach()
        return loss, {"top1": acc[1], "topk": acc[2], "n_valid": acc[3]}

    def compute_loss(self, y_hat: Tensor, y: Tensor) -> Tensor:
        raise NotImplementedError("ClassificationHead.compute_loss(logits, y): the [B, C] logits are never stored on the training "
                                  "path; use the fused entry loss_and_stats(x, y) -> (loss, stats)")

    def log_metrics(self, out: dict, log_fn, stage: str) -> None:
        """``out``: {"loss", "stats"} as ``loss_and_stats`` returns them"""
        if "stats" not in out:
            raise NotImplementedError("ClassificationHead.log_metrics takes the stats of loss_and_stats(x, y), not logits")
        log_fn(f"loss/aux/{self.head_name}/{stage}", out["loss"])
        log_fn(f"metrics/acc_top1/{self.head_name}/{stage}", out["stats"]["top1"])
        log_fn(f"metrics/acc_top{self.top_k}/{self.head_name}/{stage}", out["stats"]["topk"])


class CrossModalContrastiveHead(BaseHead):
    def __init__(self, *args, **kwargs) -> None:
        raise NotImplementedError("CrossModalContrastiveHead is not built: viscy_amd builds ClassificationHead of the auxiliary heads")
