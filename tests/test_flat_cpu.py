"""CPU: viscy_amd.flat — the flat parameter layout of every engine against tests/golden/flat_layout.json (optimiser state is
indexed by flat offset: the layout is a checkpoint format), the last-outstanding-backward rule and autograd mode on a toy engine,
and the module-side mixins on the four model classes."""

import json
import os
import types

import pytest
import torch
from torch import nn

from tests import flat_layout_cases as C
from tests import ref_ops, ref_ops_fnet3d
from viscy_amd.flat import FlatEngine, NativeModule, engine_apply

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flat_layout.json")) as _f:
    LAYOUT = json.load(_f)


# ------------------------------------------------------------------------------------------------ layout
def test_every_configuration_is_recorded():
    assert sorted(LAYOUT) == sorted(C.tags())
    assert "trainable_numel_encoder_frozen" in LAYOUT[C.FROZEN_CASE]


@pytest.mark.parametrize("tag", C.tags())
def test_layout_reproduces_the_recorded_one(tag):
    core, ops = C.make(tag)
    before = {n: p.detach().clone() for n, p in core.named_parameters()}
    eng = core.engine(ops)
    assert all(o % 4 == 0 for o in eng.offsets)  # 16-byte aligned slices
    base, n = eng.flat.data_ptr(), eng.flat.numel()
    assert len(eng.order) == len(before) == len(eng.offsets)
    name_of = {id(p): k for k, p in core.named_parameters()}
    for p, o in zip(eng.order, eng.offsets):
        assert p.data_ptr() == base + 4 * o and o + p.numel() <= n
        assert torch.equal(p.detach(), before[name_of[id(p)]])
        assert eng.g(p).data_ptr() == eng.flat_grad.data_ptr() + 4 * o and eng.g(p).shape == p.shape
    bb = eng.bucket_bounds
    assert bb[0][0] == 0 and bb[-1][1] == n and all(a[1] == b[0] for a, b in zip(bb, bb[1:]))
    assert eng.numel == sum(p.numel() for p in core.parameters())
    assert (eng.on_bucket_ready, eng._pending_bwd, eng.model, eng.ops, eng.device) == (None, 0, core, ops, torch.device("cpu"))
    assert C.record(tag, core, eng) == LAYOUT[tag]


# ------------------------------------------------------------------------------------------------ toy engine
class _ToyEngine(FlatEngine):
    name = "Toy"

    def __init__(self, model, ops=None):
        self.fail_at = None
        self.extras = []
        super().__init__(model, types.SimpleNamespace() if ops is None else ops)

    def _param_order(self):
        m = self.model
        self._bucket_marks = [0, 1, 2, 3]
        return [m.c, m.b, m.a]

    def forward(self, x, dt, need_bwd, *extra):
        self.extras.append(extra)
        if need_bwd:
            self._count_forward()
        out = x * 2.0
        return ((out, out + 1.0) if extra and extra[0] == "pair" else out), ({} if need_bwd else None)

    def backward_stages(self, sv, dout):
        d = dout if torch.is_tensor(dout) else dout[0] + 2.0 * dout[1]
        for i, p in enumerate(self.order):
            if self.fail_at == i:
                raise RuntimeError("boom")
            self.g(p).add_(d.sum() * (i + 1) * torch.arange(1.0, p.numel() + 1.0).view(p.shape))
            yield i


class _Toy(NativeModule, nn.Module):
    def __init__(self):
        super().__init__()
        self.a, self.b, self.c = nn.Parameter(torch.randn(3)), nn.Parameter(torch.randn(2, 3)), nn.Parameter(torch.randn(5))

    def _engine_class(self):
        return _ToyEngine


def test_toy_layout_and_buckets():
    m = _Toy()
    eng = m.engine()
    assert eng.offsets == [0, 8, 16] and eng.flat.numel() == 20 and eng.numel == 14 and eng.trainable_numel() == 20
    assert eng.bucket_bounds == [(0, 8), (8, 16), (16, 20)]


def test_bucket_hook_fires_in_the_last_outstanding_backward_only():
    eng = _Toy().engine()
    fired = []
    eng.on_bucket_ready = fired.append
    d = torch.ones(2)
    eng._count_forward()
    eng._count_forward()
    eng.backward({}, d)
    assert fired == []
    eng.backward({}, d)
    assert fired == [0, 1, 2]
    eng._count_forward()
    eng._count_forward()
    eng.reset_pending()  # a new step (or a driver that runs the stages itself): nothing is outstanding
    eng.backward({}, d)
    assert fired == [0, 1, 2, 0, 1, 2]
    assert eng._pending_bwd == 0


@pytest.mark.parametrize("own_zeros", [False, True], ids=["zeros_like", "ops_zeros"])
def test_autograd_mode_equals_flat_mode_from_a_zeroed_buffer(own_zeros):
    calls = []

    def zeros(*shape, device):
        calls.append(shape)
        return torch.zeros(shape, dtype=torch.float32, device=device)

    torch.manual_seed(0)
    m = _Toy()
    eng = m.engine(types.SimpleNamespace(zeros=zeros) if own_zeros else None)
    x = torch.randn(4)
    m.grad_mode = "flat"
    eng.reset_pending()
    eng.flat_grad.zero_()
    engine_apply(m, x).sum().backward()
    want = eng.flat_grad.clone()
    assert want.abs().max() > 0 and all(p.grad is eng.g(p) for p in eng.order)
    # autograd mode: the flat buffer and the map are left as they were, the gradients arrive through autograd
    m.grad_mode = "autograd"
    m.b.requires_grad_(False)
    for p in eng.order:
        p.grad = None
    eng.flat_grad.fill_(7.0)
    fg, gmap = eng.flat_grad, eng.grad_of
    engine_apply(m, x).sum().backward()
    assert eng.flat_grad is fg and eng.grad_of is gmap and bool((fg == 7.0).all())
    assert m.b.grad is None
    for p, o in zip(eng.order, eng.offsets):
        if p is not m.b:
            assert torch.equal(p.grad.flatten(), want[o : o + p.numel()])
    assert calls == ([(20,)] if own_zeros else [])
    # the engine-level form hands back None for the frozen parameter, in flat order
    eng._count_forward()
    grads = eng.backward_autograd({}, torch.ones(4) * x.numel() / 4)
    assert [g is None for g in grads] == [False, True, False] and grads[0].shape == m.c.shape


def test_autograd_mode_restores_the_buffers_when_the_backward_raises():
    m = _Toy()
    eng = m.engine()
    fg, gmap = eng.flat_grad, eng.grad_of
    eng.fail_at = 1
    y = engine_apply(m, torch.randn(4)).sum()
    with pytest.raises(RuntimeError, match="boom"):
        y.backward()
    assert eng.flat_grad is fg and eng.grad_of is gmap and float(fg.abs().max()) == 0.0
    with pytest.raises(RuntimeError, match="boom"):
        eng.backward_autograd({}, torch.ones(4))
    assert eng.flat_grad is fg and eng.grad_of is gmap


def test_engine_apply_passes_extras_through_and_takes_two_outputs():
    m = _Toy()
    eng = m.engine()
    x = torch.randn(4)
    a, b = engine_apply(m, x, "pair", 3)
    assert eng.extras[-1] == ("pair", 3) and torch.equal(b, a + 1.0)
    (a.sum() + b.sum()).backward()  # backward(ctx, *douts) with the leading Nones counted from the call
    one = _Toy()
    one.load_state_dict(m.state_dict())
    engine_apply(one, x).sum().backward()
    assert one.engine().extras[-1] == ()
    for p, q in zip(m.parameters(), one.parameters()):
        assert torch.equal(p.grad, 3.0 * q.grad)  # d = dout[0] + 2 dout[1]
    with torch.no_grad():
        y = engine_apply(m, x)
    assert not y.requires_grad and eng._pending_bwd == 0
    # a forward without bookkeeping cannot be differentiated: the message names the model
    out, sv = eng.forward(x, torch.float32, False)
    assert sv is None
    from viscy_amd.flat import _EngineFn

    ctx = types.SimpleNamespace(model=m, sv=None, n_lead=4)
    with pytest.raises(RuntimeError, match=r"viscy_amd\.Toy: backward called but the forward ran without gradient bookkeeping"):
        _EngineFn.backward(ctx, torch.ones(4))


def test_engine_names_in_the_bookkeeping_error():
    from viscy_amd import engine_unet3d, engine_unext2

    assert engine_unext2.Engine.name == "UNeXt2" and engine_unet3d.Engine.name == "Unet3d"


# ------------------------------------------------------------------------------------------------ mixins on the model classes
def _models():
    from viscy_amd.contrastive import ContrastiveEncoder
    from viscy_amd.fcmae import FullyConvolutionalMAE
    from viscy_amd.unet3d import Unet3d
    from viscy_amd.unext2 import UNeXt2

    small = dict(depths=(1, 1, 1, 1), dims=(16, 32, 64, 128))
    return {
        "UNeXt2": (UNeXt2(backbone="convnextv2_atto"), ref_ops, (1, 1, 5, 64, 64), "UNeXt2"),
        "Unet3d": (Unet3d(depth=2, mult_chan=4), ref_ops_fnet3d, (1, 1, 8, 16, 16), "Unet3d"),
        "FullyConvolutionalMAE": (FullyConvolutionalMAE(1, 1, encoder_blocks=[1, 1, 1, 1], dims=[16, 32, 64, 128]), ref_ops,
                                  (1, 1, 5, 64, 64), "_FcmaeCore"),
        "ContrastiveEncoder": (ContrastiveEncoder("convnextv2_tiny", 1, 5, embedding_dim=32, projection_dim=16, **small), ref_ops,
                               (1, 1, 5, 64, 64), "_EmbedCore"),
    }


@pytest.fixture(scope="module")
def models():
    return _models()


@pytest.mark.parametrize("which", ["UNeXt2", "Unet3d", "FullyConvolutionalMAE", "ContrastiveEncoder"])
def test_engine_is_rebuilt_after_apply_and_for_other_ops(models, which):
    m, ops, _, _ = models[which]
    core = getattr(m, "_core", m)
    assert core._engine is None and m.grad_mode == "autograd" and m.compute_dtype is None
    e1 = m.engine(ops)
    assert m.engine() is e1 and m.engine(ops) is e1 and core._engine is e1 and e1.ops is ops and e1.model is core
    other = types.SimpleNamespace(**{k: getattr(ops, k) for k in dir(ops) if not k.startswith("__")})
    e2 = m.engine(other)
    assert e2 is not e1 and e2.ops is other and m.engine() is e2
    m.float()  # nn.Module._apply: parameter storage may move, the flat views are rebuilt on the next call
    assert core._engine is None
    e3 = m.engine(ops)
    assert e3 is not e2 and all(p.data_ptr() == e3.flat.data_ptr() + 4 * o for p, o in zip(e3.order, e3.offsets))


@pytest.mark.parametrize("which", ["FullyConvolutionalMAE", "ContrastiveEncoder"])
def test_wrapper_knobs_reach_the_core(models, which):
    m = models[which][0]
    core = m._core
    assert "_core" not in dict(m.named_children()) and m.cfg is core.cfg
    try:
        m.compute_dtype, m.grad_mode = torch.bfloat16, "flat"
        assert (core.compute_dtype, core.grad_mode) == (torch.bfloat16, "flat")
        assert (m.compute_dtype, m.grad_mode) == (torch.bfloat16, "flat")
        assert "compute_dtype" not in m.__dict__ and "grad_mode" not in m.__dict__
        m.eval()
        assert not core.training and not m.training
        m.train()
        assert core.training and m.training
    finally:
        core.compute_dtype, core.grad_mode = None, "autograd"


@pytest.mark.parametrize("which", ["UNeXt2", "Unet3d", "FullyConvolutionalMAE", "ContrastiveEncoder"])
def test_cpu_input_error_message(models, which):
    m, _, shape, name = models[which]
    with pytest.raises(RuntimeError) as e:
        m(torch.zeros(shape))
    assert str(e.value) == (f"viscy_amd.{name} runs on MI355X HIP kernels only (no CPU / eager fallback): move the model "
                            "and the input to a 'cuda' (ROCm) device")


def test_state_dict_key_counts_are_unchanged():
    from viscy_amd.unext2 import UNeXt2

    assert len(UNeXt2(backbone="convnextv2_atto").state_dict()) == 213
    assert len(UNeXt2(backbone="convnextv2_tiny").state_dict()) == 273


def test_resolve_dtype(models):
    atto, unet = models["UNeXt2"][0], models["Unet3d"][0]
    fcmae = models["FullyConvolutionalMAE"][0]._core
    was = torch.is_autocast_enabled("cuda"), torch.get_autocast_dtype("cuda")
    try:
        for m in (atto, unet, fcmae):
            m.compute_dtype = torch.bfloat16
        assert not atto._bf16_ok() and atto._resolve_dtype() == torch.float32  # a 60-channel row: exact fp32 kernels instead
        assert unet._resolve_dtype() == torch.bfloat16 and fcmae._bf16_ok() and fcmae._resolve_dtype() == torch.bfloat16
        for m in (atto, unet, fcmae):
            m.compute_dtype = torch.float32
            assert m._resolve_dtype() == torch.float32
            m.compute_dtype = None
            assert m._resolve_dtype() == torch.float32
        # compute_dtype None follows autocast (the thread's autocast state is set directly: no device is needed for that)
        torch.set_autocast_enabled("cuda", True)
        torch.set_autocast_dtype("cuda", torch.bfloat16)
        assert unet._resolve_dtype() == torch.bfloat16 and fcmae._resolve_dtype() == torch.bfloat16
        assert atto._resolve_dtype() == torch.float32
        torch.set_autocast_dtype("cuda", torch.float16)
        assert unet._resolve_dtype() == torch.float32
    finally:
        torch.set_autocast_enabled("cuda", was[0])
        torch.set_autocast_dtype("cuda", was[1])
        for m in (atto, unet, fcmae):
            m.compute_dtype = None
