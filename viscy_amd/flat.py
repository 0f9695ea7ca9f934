"""What every hand-scheduled network of this package shares: the flat fp32 parameter / gradient buffers with the bookkeeping of
a training step (``FlatEngine``), the one autograd node that drives an engine (``engine_apply``), and the module-side plumbing
(``NativeModule`` for a network that owns an engine, ``CoreProxy`` for a reference-named wrapper around one).

An engine subclass states its parameter order (``_param_order``, which also fills ``_bucket_marks``) and its schedule
(``forward(x, dt, need_bwd, *extra) -> (out, saved)``, ``backward_stages(saved, dout)`` yielding each gradient bucket's index
as it completes).  ``FlatAdamW``, ``FlatDataParallel`` and ``TrainStep`` use the surface of ``FlatEngine`` and nothing else.
Adam's moments are indexed by flat offset, so the layout is a checkpoint format (pinned by tests/golden/flat_layout.json).
"""

from __future__ import annotations

import torch
from torch import Tensor

from . import _lib as L


class FlatEngine:
    name = "FlatEngine"  # the model's public name, for error messages

    def __init__(self, model, ops):
        self.model, self.ops = model, ops
        params = list(model.parameters())
        self.device = params[0].device
        # ---- flat parameter / gradient buffers, reverse forward order (gradient buckets become ready front-to-back in backward)
        order = self._param_order()
        assert len(order) == len(params) and len({id(p) for p in order}) == len(order)
        offs, off = [], 0
        for p in order:
            offs.append(off)
            off += (p.numel() + 3) // 4 * 4  # every slice 16-byte aligned
        self.flat = torch.zeros(off, dtype=torch.float32, device=self.device)
        self.flat_grad = torch.zeros(off, dtype=torch.float32, device=self.device)
        self.order, self.offsets, self.numel = order, offs, sum(p.numel() for p in order)
        with torch.no_grad():
            for p, v in zip(order, self._views(self.flat)):
                v.copy_(p.detach().to(torch.float32))
                p.data = v
        self.grad_of = self._grad_map(self.flat_grad)
        self.bucket_bounds = self._bucket_bounds()
        self.on_bucket_ready = None  # callable(bucket_index) set by viscy_amd.parallel
        self._pending_bwd = 0        # forwards of the current step whose backward has not run yet

    def _param_order(self):
        """every parameter of the model once, in backward order; appends to ``self._bucket_marks`` the index in that list at
        which each gradient bucket ends (starting with 0)"""
        raise NotImplementedError

    def _views(self, buf: Tensor):
        return [buf[o : o + p.numel()].view(p.shape) for p, o in zip(self.order, self.offsets)]

    def _grad_map(self, buf: Tensor):
        return {id(p): v for p, v in zip(self.order, self._views(buf))}

    def _bucket_bounds(self):
        b = []
        for i in range(len(self._bucket_marks) - 1):
            lo = self.offsets[self._bucket_marks[i]]
            hi_idx = self._bucket_marks[i + 1]
            hi = self.offsets[hi_idx] if hi_idx < len(self.offsets) else self.flat.numel()
            b.append((lo, hi))
        return b

    def g(self, p) -> Tensor:
        return self.grad_of[id(p)]

    def trainable_numel(self) -> int:
        """length of the prefix of the flat buffers that the optimiser updates"""
        return self.flat.numel()

    def attach_grads(self) -> None:
        for p in self.order:
            p.grad = self.grad_of[id(p)]

    # ------------------------------------------------------------------ the step's count of outstanding backwards
    def _count_forward(self) -> None:
        """a forward with gradient bookkeeping ran: its backward is outstanding"""
        self._pending_bwd += 1

    def reset_pending(self) -> None:
        """no forward is waiting for ``backward``: a new step begins, or the caller runs ``backward_stages`` itself"""
        self._pending_bwd = 0

    def backward(self, sv, dout) -> None:
        """Accumulates the parameter gradients into the flat gradient buffer (no input gradient: the image stack never
        requires grad on this path).  ``on_bucket_ready(i)`` fires as bucket i completes — but only during the LAST outstanding
        backward of the step: with several forwards per step (CombinedLoader batches, DynaCLR with unpaired forwards) an
        earlier backward leaves buckets that later ones still accumulate into."""
        last = self._pending_bwd <= 1
        self._pending_bwd = max(self._pending_bwd - 1, 0)
        for i in self.backward_stages(sv, dout):
            if last and self.on_bucket_ready:
                self.on_bucket_ready(i)

    def backward_autograd(self, sv, dout) -> tuple:
        """autograd mode: ``backward`` into a zeroed buffer of its own, whose views are handed to autograd (None for a frozen
        parameter); the flat gradient buffer is left as it was"""
        saved = self.flat_grad, self.grad_of
        try:
            zeros = getattr(self.ops, "zeros", None)  # the HIP backend's own fill: no ATen launch
            self.flat_grad = zeros(saved[0].numel(), device=saved[0].device) if zeros else torch.zeros_like(saved[0])
            self.grad_of = self._grad_map(self.flat_grad)
            self.backward(sv, dout)
            return tuple(self.grad_of[id(p)] if p.requires_grad else None for p in self.order)
        finally:
            self.flat_grad, self.grad_of = saved


class _EngineFn(torch.autograd.Function):
    """the whole network as one autograd node: ``rest`` = what the engine's forward takes after ``need_bwd``, then the
    parameters in flat order (so that autograd calls ``backward`` and, in autograd mode, receives their gradients)"""

    @staticmethod
    def forward(ctx, x, model, dt, need_bwd, *rest):
        eng = model.engine()
        ctx.n_lead = 4 + len(rest) - len(eng.order)
        out, sv = eng.forward(x, dt, need_bwd, *rest[: len(rest) - len(eng.order)])
        ctx.model, ctx.sv = model, sv
        return out

    @staticmethod
    def backward(ctx, *douts):
        dout = douts[0] if len(douts) == 1 else douts  # the embedding tail returns (embedding, projection)
        model, sv = ctx.model, ctx.sv
        eng = model.engine()
        if sv is None:
            raise RuntimeError(f"viscy_amd.{eng.name}: backward called but the forward ran without gradient bookkeeping")
        ctx.sv = None
        lead = (None,) * ctx.n_lead
        if model.grad_mode == "flat":
            eng.backward(sv, dout)
            return lead + (None,) * len(eng.order)
        return lead + eng.backward_autograd(sv, dout)


def engine_apply(model, x: Tensor, *extra):
    """``model``'s engine forward on ``x`` (prepared by the caller) under autograd; ``extra`` goes through to ``Engine.forward``"""
    eng = model.engine()
    dt = model._resolve_dtype()
    if model.grad_mode == "flat":
        eng.attach_grads()
    need_bwd = torch.is_grad_enabled() and any(p.requires_grad for p in eng.order)
    with torch.autocast("cuda", enabled=False):
        return _EngineFn.apply(x, model, dt, need_bwd, *extra, *eng.order)


# ------------------------------------------------------------------------------------------------ module side
class NativeModule:
    """Mixin (in front of ``nn.Module``) of a network that runs on its own ``FlatEngine``."""

    compute_dtype: torch.dtype | None = None  # None: bf16 under torch.autocast(bfloat16), fp32 otherwise
    grad_mode = "autograd"  # or "flat": gradients are written straight into the flat buffer
    _engine = None

    def _engine_class(self):
        raise NotImplementedError

    def _bf16_ok(self) -> bool:
        return True

    def _resolve_dtype(self) -> torch.dtype:
        want = self.compute_dtype
        if want is None:
            want = torch.bfloat16 if torch.is_autocast_enabled() and torch.get_autocast_dtype("cuda") == torch.bfloat16 else torch.float32
        if want == torch.bfloat16 and not self._bf16_ok():
            return torch.float32  # e.g. convnextv2_atto: exact fp32 kernels instead of failing on a 60-channel row
        return want

    def engine(self, ops=None):
        dev = next(self.parameters()).device
        if self._engine is None or self._engine.device != dev or (ops is not None and self._engine.ops is not ops):
            self._engine = self._engine_class()(self, ops)
        return self._engine

    def _apply(self, fn, *a, **k):
        self._engine = None  # parameter storage moves: flat views must be rebuilt
        return super()._apply(fn, *a, **k)

    def _require_hip(self, x: Tensor) -> None:
        if not x.is_cuda:
            raise RuntimeError(
                f"viscy_amd.{type(self).__name__} runs on MI355X HIP kernels only (no CPU / eager fallback): move the model "
                "and the input to a 'cuda' (ROCm) device"
            )
        L.lib()  # raises loudly when libvsx.so is missing


class CoreProxy:
    """Mixin (in front of ``nn.Module``) of a reference-named parameter tree around a ``NativeModule`` kept in ``_core``
    (set with ``object.__setattr__``: NOT a registered submodule): the engine's knobs live on the core."""

    @property
    def cfg(self):
        return self._core.cfg

    @property
    def compute_dtype(self):
        return self._core.compute_dtype

    @compute_dtype.setter
    def compute_dtype(self, v):
        self._core.compute_dtype = v

    @property
    def grad_mode(self):
        return self._core.grad_mode

    @grad_mode.setter
    def grad_mode(self, v):
        self._core.grad_mode = v

    def engine(self, ops=None):
        return self._core.engine(ops)

    def _apply(self, fn, *a, **k):
        self._core._engine = None  # parameter storage moves: flat views must be rebuilt
        return super()._apply(fn, *a, **k)

    def train(self, mode: bool = True):
        self._core.train(mode)  # stochastic depth / BatchNorm mode: the engine reads the core's flag
        return super().train(mode)
