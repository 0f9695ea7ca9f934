"""CPU: the public surface of the DynaCLR triplet branch (viscy_amd.contrastive.TripletMarginLoss and its wiring into
ContrastiveModule / viscy_amd.config) — what is accepted, what is refused and how; no kernel runs here.  The three-view
trunk pass is checked at schedule level (kernels = tests/ref_ops.py) against three separate forwards of the oracle."""

import pytest
import torch
from torch import nn

SMALL = dict(embedding_dim=32, projection_dim=16, depths=(1, 1, 1, 1), dims=(16, 32, 48, 64))


def _module(**kw):
    from viscy_amd.contrastive import ContrastiveEncoder, ContrastiveModule

    enc = ContrastiveEncoder("convnextv2_tiny", in_channels=1, in_stack_depth=5, **SMALL)
    return ContrastiveModule(enc, example_input_array_shape=(1, 1, 5, 32, 32), **kw)


def test_constructor_has_torch_keywords_and_refuses_what_is_not_built():
    from viscy_amd.contrastive import TripletMarginLoss

    ours, theirs = TripletMarginLoss(), nn.TripletMarginLoss()
    for k in ("margin", "p", "eps", "swap", "reduction"):
        assert getattr(ours, k) == getattr(theirs, k), k
    loss = TripletMarginLoss(margin=0.5, p=2, eps=1e-5, swap=False, reduction="sum")
    assert (loss.margin, loss.p, loss.eps, loss.swap, loss.reduction) == (0.5, 2.0, 1e-5, False, "sum")
    assert loss.last_stats is None
    with pytest.raises(NotImplementedError, match="p=1"):
        TripletMarginLoss(p=1)
    with pytest.raises(NotImplementedError, match="swap"):
        TripletMarginLoss(swap=True)
    with pytest.raises(NotImplementedError, match="none"):
        TripletMarginLoss(reduction="none")
    with pytest.raises(ValueError, match="reduction"):
        TripletMarginLoss(reduction="median")
    import viscy_amd

    assert viscy_amd.TripletMarginLoss is TripletMarginLoss


def test_forward_validates_shapes_and_has_no_cpu_fallback():
    from viscy_amd.contrastive import TripletMarginLoss

    loss = TripletMarginLoss(margin=0.5)
    a = torch.zeros(4, 8)
    with pytest.raises(RuntimeError, match="runs on MI355X HIP kernels only"):
        loss(a, a, a)
    for bad in ((a, a, torch.zeros(4, 7)), (a, torch.zeros(3, 8), a), (torch.zeros(8), torch.zeros(8), torch.zeros(8)),
                (torch.zeros(2, 2, 2),) * 3, (torch.zeros(0, 8),) * 3):
        with pytest.raises(ValueError, match="equal shape"):
            loss(*bad)


def test_module_takes_the_reference_default_loss():
    """the reference's `ContrastiveModule(encoder)` default, and what `class_path: torch.nn.TripletMarginLoss` produces"""
    from viscy_amd.contrastive import NTXentLoss, TripletMarginLoss

    mod = _module(loss_function=nn.TripletMarginLoss(margin=0.5))
    assert type(mod.loss_function) is TripletMarginLoss and mod.loss_function.margin == 0.5
    assert mod.loss_function.reduction == "mean" and mod.loss_function.eps == 1e-6
    mod = _module(loss_function=nn.TripletMarginLoss(margin=0.25, eps=1e-5, reduction="sum"))
    assert (mod.loss_function.margin, mod.loss_function.eps, mod.loss_function.reduction) == (0.25, 1e-5, "sum")
    ours = TripletMarginLoss(margin=0.7)
    assert _module(loss_function=ours).loss_function is ours
    assert type(_module().loss_function) is NTXentLoss   # the default here stays NT-Xent
    for unbuilt in (nn.TripletMarginLoss(swap=True), nn.TripletMarginLoss(p=1.0), nn.TripletMarginLoss(reduction="none")):
        with pytest.raises(NotImplementedError):
            _module(loss_function=unbuilt)
    with pytest.raises(NotImplementedError, match="gather_embeddings"):
        _module(loss_function=ours, gather_embeddings=True)
    mod = _module(loss_function=ours)
    mod.on_train_epoch_start()   # no temperature to schedule or log
    assert "hparams/temperature" not in mod.logged


def test_cosine_embedding_loss_is_still_refused_and_says_why():
    with pytest.raises(NotImplementedError, match="target"):
        _module(loss_function=nn.CosineEmbeddingLoss())
    with pytest.raises(NotImplementedError, match="MSELoss"):
        _module(loss_function=nn.MSELoss())


def test_config_maps_the_torch_class_path():
    from viscy_amd import config
    from viscy_amd.contrastive import ContrastiveModule, TripletMarginLoss

    node = {"class_path": "torch.nn.TripletMarginLoss", "init_args": {"margin": 0.5}}
    loss = config.instantiate(node)
    assert type(loss) is TripletMarginLoss and loss.margin == 0.5
    assert config._resolve("torch.nn.modules.loss.TripletMarginLoss") is TripletMarginLoss
    mod = config.instantiate({
        "class_path": "dynaclr.engine.ContrastiveModule",
        "init_args": {"encoder": {"class_path": "viscy_models.contrastive.ContrastiveEncoder",
                                  "init_args": dict(backbone="convnextv2_tiny", in_channels=1, in_stack_depth=5,
                                                    **{k: list(v) if isinstance(v, tuple) else v for k, v in SMALL.items()})},
                      "loss_function": node, "example_input_array_shape": [1, 1, 5, 32, 32]}})
    assert type(mod) is ContrastiveModule and type(mod.loss_function) is TripletMarginLoss and mod.triplet


def test_triplet_step_needs_the_negative_view():
    mod = _module(loss_function=nn.TripletMarginLoss(margin=0.5))
    x = torch.zeros(2, 1, 5, 32, 32)
    for step in (mod.training_step, mod.validation_step):
        with pytest.raises(KeyError, match="negative"):
            step({"anchor": x, "positive": x}, 0)


def test_three_view_pass_equals_three_calls_at_schedule_level():
    """one trunk pass over [anchor; positive; negative] with three BatchNorm groups == three separate forwards of the oracle:
    projections and the running statistics after three updates in view order"""
    from oracle import contrastive_ref as C
    from tests import ref_ops
    from tests.conftest import load_golden
    from viscy_amd.contrastive import ContrastiveEncoder
    from viscy_amd.engine_unext2 import Engine

    gold = load_golden("contrastive.pt")["v1_small_z5"]
    ref = C.randomize_encoder_(C.ContrastiveEncoder(**gold["kwargs"], **gold["arch"]), seed=gold["seed"]).train()
    mine = ContrastiveEncoder(**gold["kwargs"], **gold["arch"])
    mine.load_state_dict(ref.state_dict(), strict=True)
    mine.train()
    g = torch.Generator().manual_seed(8)
    a = torch.randn(3, 1, 5, 64, 64, generator=g)
    views = (a, a + 0.3 * torch.randn(a.shape, generator=g), torch.randn(a.shape, generator=g) * 2 + 1)
    with torch.no_grad():
        (emb, proj), _ = Engine(mine._core, ops=ref_ops).forward(torch.cat(views), torch.float32, need_bwd=False, bn_groups=3)
        outs = [ref(v) for v in views]
    er, pr = torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])
    torch.testing.assert_close(proj, pr, rtol=2e-4, atol=1e-4 * pr.abs().max().item())
    torch.testing.assert_close(emb, er, rtol=2e-4, atol=1e-4 * er.abs().max().item())
    seen = 0
    for k, v in ref.state_dict().items():
        if "running" in k or "num_batches" in k:
            seen += 1
            torch.testing.assert_close(mine.state_dict()[k].float(), v.float(), rtol=1e-4, atol=1e-5)
    assert seen == 6 and int(mine.state_dict()["projection.1.num_batches_tracked"]) == 3


def test_abi_refuses_bad_arguments_before_any_launch():
    """B < 1, D < 1 and an unknown reduction come back non-zero with vsx_last_error set; nothing reaches a kernel"""
    import ctypes

    from viscy_amd import _lib

    l = _lib.lib()
    buf = ctypes.addressof((ctypes.c_float * 8)())   # non-NULL stand-in: refused calls dereference nothing
    for B, D, red, msg in ((0, 4, 0, b"bad arguments"), (4, 0, 1, b"bad arguments"), (4, 4, 2, b"unknown reduction 2")):
        assert l.vsx_triplet_fwd(buf, buf, buf, buf, buf, B, D, 0.5, 1e-6, red, None) != 0
        assert l.vsx_last_error().startswith(b"vsx_triplet_fwd: " + msg), l.vsx_last_error()
        assert l.vsx_triplet_bwd(buf, buf, buf, buf, buf, buf, buf, buf, B, D, 0.5, 1e-6, red, None) != 0
        assert l.vsx_last_error().startswith(b"vsx_triplet_bwd: " + msg), l.vsx_last_error()
    assert l.vsx_triplet_fwd(None, buf, buf, buf, buf, 4, 4, 0.5, 1e-6, 0, None) != 0
