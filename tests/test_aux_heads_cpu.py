"""CPU: the DynaCLR auxiliary heads (viscy_amd.heads, their wiring into ContrastiveModule / viscy_amd.config / the optimiser) —
the restatement of tests/ref_aux_heads.py against the reference's recorded values (tests/golden/aux_heads.pt), the public
surface (keywords, defaults, state-dict keys, what is refused and how), and the head schedule on the CPU backend
(tests/ref_ops_aux_head.py) behind the SMALL trunk against torch autograd over the oracle encoder plus the restatement.
No kernel runs here."""

import inspect
import math
import os

import pytest
import torch
import yaml

from tests import ref_aux_heads as RA
from tests.conftest import GOLDEN, load_golden


def _close(got, ref, rtol, what):
    ref = torch.as_tensor(ref, dtype=torch.float64)
    torch.testing.assert_close(torch.as_tensor(got, dtype=torch.float64), ref, rtol=rtol, atol=1e-7 + rtol * ref.abs().max().item(),
                               msg=lambda m: f"{what}: {m}")


# ------------------------------------------------------------------------------------------------ the reference pin
@pytest.mark.parametrize("name", list(RA.KERNEL_CASES))
def test_restated_classifier_equals_the_reference_record(name):
    """the restated classifiers + cross-entropy + accuracies give what the reference's modules gave (fp64: to round-off; fp32:
    within fp32's own error), so the GPU tests may compare against the restatement in float64"""
    gold = load_golden("aux_heads.pt")["kernel"][name]
    inp = RA.build_kernel_case(name)
    for dtype, tag, rtol in ((torch.float64, "fp64", 1e-10), (torch.float32, "fp32", 1e-4)):
        ref, g = RA.kernel_reference(inp, dtype), gold[tag]
        assert abs(float(ref["loss"]) - g["loss"]) <= rtol * abs(g["loss"]), (name, tag)
        assert float(ref["top1"]) == g["top1"] and float(ref["topk"]) == g["topk"], (name, tag)   # the rank agrees with argmax / topk
        assert abs(float(ref["logits"].double().sum()) - g["checksum"]) <= rtol * g["abs_checksum"]
        for key in ("dh", "dW", "dlog_scale" if inp["mode"] == "cosine" else "dbias"):
            full = ref[key].reshape(-1)
            _close(full[RA.grad_sample_index(full.numel())], g[key], rtol, f"{name} {tag} {key}")


@pytest.mark.parametrize("name", list(RA.HEAD_CASES))
def test_restated_head_equals_the_reference_record(name):
    gold = load_golden("aux_heads.pt")["head"][name]
    case = RA.build_head_case(name)
    pick = lambda t: t.reshape(-1)[RA.grad_sample_index(t.numel())]  # noqa: E731
    for dtype, tag, rtol in ((torch.float64, "fp64", 1e-9), (torch.float32, "fp32", 2e-4)):
        ref, g = RA.head_reference(case, dtype), gold[tag]
        assert abs(float(ref["loss"]) - g["loss"]) <= rtol * abs(g["loss"])
        k = case["k"]
        hn = RA.HEAD_CASES[name]["kwargs"]["head_name"]
        assert g["logged"] == {f"loss/aux/{hn}/train": g["loss"], f"metrics/acc_top1/{hn}/train": float(ref["top1"]),
                               f"metrics/acc_top{k}/{hn}/train": float(ref["topk"])}
        _close(pick(ref["dx"]), g["dx"], rtol, f"{name} {tag} dx")
        assert sorted(ref["grads"]) == sorted(g["grads"]) and sorted(ref["buffers"]) == sorted(g["buffers"])
        for key, v in g["grads"].items():
            _close(pick(ref["grads"][key]), v, rtol, f"{name} {tag} {key}")
        for key, v in g["buffers"].items():
            _close(pick(ref["buffers"][key]), v, rtol, f"{name} {tag} {key}")


def test_keywords_defaults_keys_and_schedule_are_the_references():
    from viscy_amd import heads as H

    gold = load_golden("aux_heads.pt")
    for cls in ("BaseHead", "ClassificationHead", "CosineClassifier", "MLP"):
        sig = [(n, None if p.default is inspect.Parameter.empty else repr(p.default))
               for n, p in inspect.signature(getattr(H, cls).__init__).parameters.items() if n != "self"]
        assert sig == gold["signatures"][cls], cls
    assert list(H.ClassificationHead("h", "k", 8, 256, 7).state_dict()) == gold["state_dict_keys"]["256"]
    assert list(H.ClassificationHead("h", "k", 8, [64, 32], 7, cosine_classifier=False).state_dict()) == gold["state_dict_keys"]["[64, 32]"]
    assert "mlp.backbone.4.num_batches_tracked" in gold["state_dict_keys"]["[64, 32]"] and "mlp.head.log_scale" in gold["state_dict_keys"]["256"]
    for make in (H.ClassificationHead, RA.ClassificationHead):
        head = make(**RA.OPS_HEAD)
        assert head.get_weight() == gold["ops_schedule"]["initial"] == 0.0
        for e in RA.SCHEDULE_EPOCHS:
            head.step(e)
            assert head.get_weight() == gold["ops_schedule"][e], e
    assert gold["ops_schedule"][15] == pytest.approx(0.25, rel=1e-12) and gold["ops_schedule"][30] == gold["ops_schedule"][31] == 0.5
    const = H.ClassificationHead("h", "k", 8, 8, 7, loss_weight=0.3)
    const.step(7)
    assert const.get_weight() == 0.3


def test_initialisation_is_the_references():
    """same seed, same parameters as the restatement (whose construction order the golden pins through the head cases)"""
    from viscy_amd.heads import ClassificationHead

    for name, c in RA.HEAD_CASES.items():
        torch.manual_seed(c["seed"])
        mine = ClassificationHead(**c["kwargs"])
        torch.manual_seed(c["seed"])
        ref = RA.ClassificationHead(**c["kwargs"])
        for (k, a), (k2, b) in zip(mine.state_dict().items(), ref.state_dict().items()):
            assert k == k2 and torch.equal(a, b), (name, k)
    head = ClassificationHead("h", "k", 16, 8, 5)
    assert float(head.mlp.head.log_scale.detach()) == pytest.approx(math.log(20.0), rel=1e-7) and head.mlp.head.weight.std() < 0.02


# ------------------------------------------------------------------------------------------------ refusals
def test_what_is_not_built_refuses_itself_by_name():
    from viscy_amd import heads as H

    with pytest.raises(NotImplementedError, match="projection mode"):
        H.MLP(16, 8, out_dims=4)
    with pytest.raises(ValueError, match="out_dims is required"):
        H.MLP(16, 8)
    with pytest.raises(NotImplementedError, match="dropout"):
        H.MLP(16, 8, num_classes=3, dropout=0.1)
    for act in ("gelu", "silu"):
        with pytest.raises(NotImplementedError, match=act):
            H.MLP(16, 8, num_classes=3, activation=act)
    with pytest.raises(ValueError, match="activation"):
        H.MLP(16, 8, num_classes=3, activation="tanh")
    with pytest.raises(NotImplementedError, match="norm='ln'"):
        H.MLP(16, 8, num_classes=3, norm="ln")
    with pytest.raises(NotImplementedError, match="CrossModalContrastiveHead"):
        H.CrossModalContrastiveHead("x", "X_pls", in_dims=16, target_dims=8)
    for bad in (dict(in_dims=18, hidden_dims=8), dict(in_dims=16, hidden_dims=6), dict(in_dims=16, hidden_dims=[8, 10])):
        with pytest.raises(NotImplementedError, match="multiples of 4"):
            H.ClassificationHead("h", "k", num_classes=3, top_k=1, **bad)
    with pytest.raises(ValueError, match="top_k"):
        H.ClassificationHead("h", "k", 16, 8, num_classes=3, top_k=4)
    with pytest.raises(ValueError, match="top_k"):
        H.ClassificationHead("h", "k", 16, 8, num_classes=3, top_k=0)


def test_entry_points_have_no_cpu_fallback_and_no_silent_gradient_loss():
    from viscy_amd.heads import ClassificationHead

    head = ClassificationHead("h", "k", 16, 8, num_classes=3, top_k=2)
    x, y = torch.zeros(4, 16), torch.zeros(4, dtype=torch.long)
    with pytest.raises(RuntimeError, match="runs on MI355X HIP kernels only"):
        head.loss_and_stats(x, y)
    with pytest.raises(RuntimeError, match="runs on MI355X HIP kernels only"):
        head(x)
    with pytest.raises(RuntimeError, match="gradient"):
        head(x.clone().requires_grad_(True))
    with pytest.raises(NotImplementedError, match="loss_and_stats"):
        head.compute_loss(torch.zeros(4, 3), y)
    with pytest.raises(NotImplementedError, match="loss_and_stats"):
        head.log_metrics({"loss": x.sum(), "logits": torch.zeros(4, 3), "y": y}, print, "train")
    for bad_x, bad_y in ((torch.zeros(4, 12), y), (x, torch.zeros(3, dtype=torch.long)), (x, torch.zeros(4)), (x, torch.zeros(4, 2, dtype=torch.long))):
        with pytest.raises(ValueError):
            head.loss_and_stats(bad_x, bad_y)


def test_abi_refuses_unserved_shapes_before_any_launch():
    import ctypes

    from viscy_amd import _lib

    l = _lib.lib()
    buf = ctypes.addressof((ctypes.c_float * 64)()) // 16 * 16 + 16   # non-NULL, 16-byte aligned stand-in: refused calls read nothing
    fwd = lambda B, H, C, k, splits=0: l.vsx_cls_ce_fwd(buf, buf, buf, None, None, None, buf, B, H, C, k, splits, buf, buf, buf, 1 << 30, None)  # noqa: E731
    for args, msg in (((4, 6, 3, 1), b"H=6 must be a multiple of 4"), ((4, 0, 3, 1), b"H=0"), ((0, 4, 3, 1), b"B=0"), ((4, 4, 0, 1), b"C=0"),
                      ((4, 4, 3, 0), b"k=0 must be in [1, C=3]"), ((4, 4, 3, 4), b"k=4 must be in [1, C=3]"), ((4, 4, 3, 1, -1), b"splits=-1")):
        assert fwd(*args) != 0
        assert l.vsx_last_error().startswith(b"vsx_cls_ce_fwd: " + msg), l.vsx_last_error()
    assert l.vsx_cls_ce_fwd(buf, buf, buf, buf, None, None, None, 4, 4, 3, 1, 0, buf, buf, buf, 1 << 30, None) != 0   # half a cosine classifier
    assert l.vsx_cls_ce_fwd(buf, buf, buf, None, None, None, None, 4, 4, 3, 1, 0, buf, buf, buf, 8, None) != 0         # workspace too small
    assert b"vsx_cls_ce_fwd_ws_bytes" in l.vsx_last_error()
    assert l.vsx_cls_ce_fwd_ws_bytes(4, 4, 3) == (1 * 4 * 3 + 4) * 4 and l.vsx_cls_ce_fwd_ws_bytes(4, 6, 3) == 0
    assert l.vsx_cls_ce_bwd_ws_bytes(5, 4, 3) == (16 + 12 + 5) * 4
    assert l.vsx_cls_logits(buf, buf, None, None, None, None, 4, 6, 3, buf, None) != 0
    assert l.vsx_cls_ce_bwd(buf, buf, buf, None, None, None, None, buf, buf, buf, 4, 6, 3, buf, buf, None, None, buf, 1 << 30, None) != 0
    assert l.vsx_cls_ce_bwd(buf, buf, buf, None, None, None, None, buf, buf, buf, 4, 4, 3, buf, buf, None, buf, buf, 1 << 30, None) != 0
    assert b"cosine takes dlog_scale" in l.vsx_last_error()
    assert l.vsx_cls_inv_norm(None, buf, 4, 4, None) != 0


# ------------------------------------------------------------------------------------------------ module, config, optimiser
def _module(**kw):
    from viscy_amd.contrastive import ContrastiveEncoder, ContrastiveModule

    enc = ContrastiveEncoder("convnextv2_tiny", in_channels=1, in_stack_depth=5, **RA.SMALL)
    return ContrastiveModule(enc, example_input_array_shape=(1, 1, 5, 32, 32), **kw)


def test_auxiliary_heads_reach_the_module():
    from viscy_amd.heads import ClassificationHead

    head = ClassificationHead(**RA.MODULE_HEAD)
    mod = _module(auxiliary_heads={"gene": head})
    assert mod.auxiliary_heads["gene"] is head
    keys = [k for k in mod.state_dict() if k.startswith("auxiliary_heads.")]
    assert keys == ["auxiliary_heads.gene." + k for k in head.state_dict()] and len(keys) == 9
    assert len(_module().auxiliary_heads) == 0 and _module().heads_engine() is None
    with pytest.raises(NotImplementedError, match="projection"):
        _module(projection=torch.nn.Linear(4, 4))
    with pytest.raises(TypeError, match="BaseHead"):
        _module(auxiliary_heads={"gene": torch.nn.Linear(4, 4)})
    # the heads' parameters share ONE flat buffer of their own; the encoder's flat layout is untouched
    two = _module(auxiliary_heads={"gene": ClassificationHead(**RA.MODULE_HEAD),
                                   "marker": ClassificationHead("marker", "marker_label", 64, [8], 5, cosine_classifier=False, top_k=2)})
    eng = two.heads_engine()
    assert eng is two.heads_engine() and all(h._engine is eng for h in two.auxiliary_heads.values())
    n_params = sum(p.numel() for p in two.auxiliary_heads.parameters())
    assert eng.numel == n_params and len(eng.order) == len(list(two.auxiliary_heads.parameters())) and len(eng.bucket_bounds) == 1
    base = eng.flat.data_ptr()
    assert all(base <= p.data_ptr() < base + 4 * eng.flat.numel() for p in two.auxiliary_heads.parameters())
    assert two.model.engine().flat.numel() == _module().model.engine().flat.numel()
    with pytest.raises(NotImplementedError, match="auxiliary heads run on the eager step"):
        two.make_train_step(None)
    # the weight schedule is stepped and logged at the start of an epoch
    sched = _module(auxiliary_heads={"gene": ClassificationHead(**dict(RA.OPS_HEAD, in_dims=64))})
    for epoch in (0, 15, 30):
        sched.current_epoch = epoch
        sched.on_train_epoch_start()
    assert sched.logged["hparams/loss_weight/gene"] == [0.0, pytest.approx(0.25, rel=1e-12), 0.5]


def test_labels_come_from_the_batch_then_from_the_metadata():
    mod = _module()
    a = torch.zeros(3, 1, 5, 32, 32)
    y = torch.tensor([2, 0, 1])
    assert mod._get_labels({"anchor": a, "gene_label": y}, "gene_label") is y
    meta = [{"labels": {"gene_label": int(v)}} for v in y]
    got = mod._get_labels({"anchor": a, "anchor_meta": meta}, "gene_label")
    assert got.dtype == torch.long and torch.equal(got, y)
    assert mod._get_labels({"anchor": a, "gene_label": y * 0, "anchor_meta": meta}, "gene_label").sum() == 0   # the batch key wins
    assert mod._get_labels({"anchor": a, "anchor_meta": meta}, "other") is None
    assert mod._get_labels({"anchor": a}, "gene_label") is None and mod._get_labels({"anchor": a, "anchor_meta": [{}] * 3}, "gene_label") is None
    with pytest.raises(NotImplementedError, match="vector-valued"):
        mod._get_labels({"anchor": a, "anchor_meta": [{"labels": {"X_pls": [0.1, 0.2]}}] * 3}, "X_pls")
    with pytest.raises(NotImplementedError, match="vector-valued"):
        mod._get_labels({"anchor": a, "X_pls": torch.zeros(3, 4)}, "X_pls")


def test_config_maps_the_head_and_builds_the_ops_recipe_model():
    from viscy_amd import config, heads
    from viscy_amd.contrastive import ContrastiveModule, NTXentLoss

    gold = load_golden("aux_heads.pt")
    assert config._resolve("viscy_models.components.heads.ClassificationHead") is heads.ClassificationHead
    for name in gold["package_exports"]:   # what the reference's components/__init__.py re-exports
        assert config._resolve("viscy_models.components." + name) is getattr(heads, name)
    with pytest.raises(NotImplementedError, match="CrossModalContrastiveHead"):
        config.instantiate({"class_path": "viscy_models.components.heads.CrossModalContrastiveHead",
                            "init_args": {"head_name": "x", "batch_key": "X", "in_dims": 8, "target_dims": 4}})
    with pytest.raises(NotImplementedError, match="projection mode"):
        config.instantiate({"class_path": "viscy_models.components.heads.MLP", "init_args": {"in_dims": 8, "hidden_dims": 8, "out_dims": 4}})
    with open(os.path.join(GOLDEN, "ops_1000genes_lite_model.yml")) as f:
        mod = config.instantiate(yaml.safe_load(f)["model"])
    assert type(mod) is ContrastiveModule and type(mod.loss_function) is NTXentLoss and mod.lr == 0.0002
    head = mod.auxiliary_heads["gene"]
    assert type(head) is heads.ClassificationHead and (head.batch_key, head.top_k, head.loss_weight) == ("gene_label", 5, 0.5)
    assert head.mlp.head.weight.shape == (1001, 256) and head.mlp.backbone[0].weight.shape == (256, 768) and head.mlp.cosine
    assert (head.weight_schedule, head.weight_start, head.weight_warmup_epochs, head.get_weight()) == ("cosine", 0.0, 30, 0.0)


def test_optimiser_without_heads_is_unchanged_and_with_heads_is_one_object():
    from viscy_amd.heads import ClassificationHead
    from viscy_amd.optim import FlatAdamW, MultiFlatAdamW

    mod = _module(lr=3e-4)
    opt = mod.configure_optimizers(t_total=5)
    assert type(opt) is FlatAdamW and sorted(opt.state_dict()) == ["m", "t", "v"]
    assert opt.engine is mod.model.engine() and opt.m.numel() == mod.model.engine().flat.numel()
    mod = _module(lr=3e-4, auxiliary_heads={"gene": ClassificationHead(**RA.MODULE_HEAD)})
    opt = mod.configure_optimizers(t_total=5)
    assert type(opt) is MultiFlatAdamW and isinstance(opt, FlatAdamW) and opt.engine is mod.model.engine()
    assert [e[0] for e in opt.extra] == [mod.heads_engine()] and opt.extra[0][2].numel() == mod.heads_engine().flat.numel()
    assert opt.step_dev.numel() == 1 and opt.hyper.numel() == 8        # one step count, one hyper-parameter block for both buffers
    assert mod.auxiliary_heads["gene"].grad_mode == "flat" and mod.model.grad_mode == "flat"
    sd = opt.state_dict()
    assert sorted(sd) == ["extra", "m", "t", "v"] and sorted(sd["extra"][0]) == ["m", "v"]
    sd["extra"][0]["m"].fill_(2.0)
    fresh = mod.configure_optimizers(t_total=5)
    fresh.load_state_dict({"m": sd["m"], "v": sd["v"], "t": 3, "extra": [{k: v.clone() for k, v in sd["extra"][0].items()}]})
    assert fresh.t == 3 and float(fresh.extra[0][2].min()) == 2.0


# ------------------------------------------------------------------------------------------------ schedule level
def test_head_schedule_behind_the_small_trunk_matches_torch_autograd():
    """ContrastiveModule.training_step with both engines on the CPU backend (NT-Xent from the oracle, as no kernel runs here)
    == torch autograd over the oracle encoder plus the restated head: the loss, every logged key, the gradients of every
    trunk and head parameter, the head's running statistics"""
    from oracle import contrastive_ref as C
    from tests import ref_ops_aux_head as RO
    from viscy_amd.contrastive import ContrastiveEncoder, ContrastiveModule
    from viscy_amd.heads import ClassificationHead

    o = RA.oracle_module_step("ntxent")
    assert o["label_gap"] >= 0.05   # no label's logit near another: the accuracies do not hinge on round-off
    enc = ContrastiveEncoder("convnextv2_tiny", in_channels=1, in_stack_depth=5, **RA.SMALL)
    enc.load_state_dict(o["start"]["enc"], strict=True)
    head = ClassificationHead(**RA.MODULE_HEAD)
    head.load_state_dict(o["start"]["head"], strict=True)
    mod = ContrastiveModule(enc, example_input_array_shape=(1, 1, 5, 32, 32), auxiliary_heads={"gene": head}).train()
    enc.compute_dtype = torch.float32
    enc.engine(ops=RO)
    enc._core._require_hip = lambda x: None
    assert mod.heads_engine(ops=RO).ops is RO
    mod.loss_function = C.NTXentLoss(temperature=RA.TEMPERATURE)
    batch = {k: v for k, v in o["batch"].items() if k != "negative"}
    for paired in (True, False):
        mod.paired_forward, mod.logged = paired, {}
        for p in mod.parameters():
            p.grad = None
        head.load_state_dict(o["start"]["head"], strict=True)   # the running statistics start over
        enc.load_state_dict(o["start"]["enc"], strict=True)
        loss = mod.training_step(batch, 0)
        loss.backward()
        assert abs(loss.item() - o["total"].item()) <= 2e-4 * abs(o["total"].item()), (paired, loss.item(), o["total"].item())
        assert sorted(mod.logged) == sorted(o["logged"])
        for k, v in o["logged"].items():
            got = float(mod.logged[k][0])
            assert got == float(v) if "acc_top" in k else abs(got - float(v)) <= 2e-4 * abs(float(v)), (k, got, float(v))
        for group, named in (("enc", enc.named_parameters()), ("head", head.named_parameters())):
            for name, prm in named:
                ref = o["grads"][group][name]
                assert prm.grad is not None, name
                torch.testing.assert_close(prm.grad, ref, rtol=2e-3, atol=1e-6 + 2e-3 * ref.abs().max().item(),
                                           msg=lambda m: f"{group} {name} (paired={paired}): {m}")
        assert int(head.mlp.backbone[1].num_batches_tracked) == int(o["start"]["head"]["mlp.backbone.1.num_batches_tracked"]) + 1
    # validation: no gradient bookkeeping, running statistics, the same keys under /val
    mod.eval()
    mod.logged = {}
    with torch.no_grad():
        mod.validation_step(batch, 0)
    assert sorted(mod.logged) == sorted(k.replace("/train", "/val") for k in o["logged"])
    # a head whose key the batch does not carry is skipped: the contrastive loss alone
    mod.train()
    mod.logged = {}
    alone = mod.training_step({k: v for k, v in batch.items() if k != "gene_label"}, 0)
    assert sorted(mod.logged) == ["loss/train"] and alone.item() == mod.logged["loss/train"][0].item()


# ------------------------------------------------------------------------------------------------ the CPU backend's own statement
def _run_cpu_backend(inp, y=None):
    from tests import ref_ops_aux_head as RO

    h, W = inp["h"], inp["W"]
    y = inp["y"] if y is None else y
    if "log_scale" in inp:
        cls = dict(inv_h=RO.cls_inv_norm(h), inv_w=RO.cls_inv_norm(W), log_scale=inp["log_scale"].view(1))
        grads = dict(dlog_scale=torch.zeros(1))
    else:
        cls, grads = dict(bias=inp["bias"]), dict(dbias=torch.zeros(W.shape[0]))
    rows, acc = RO.cls_ce_fwd(h, W, y, inp["k"], **cls)
    dW = torch.zeros_like(W)
    dh = RO.cls_ce_bwd(h, W, y, rows, acc, torch.tensor([RA.GOUT]), dW, **cls, **grads)
    return dict(rows=rows, acc=acc, dh=dh, dW=dW, **{k: v.reshape(inp[k[1:]].shape) for k, v in grads.items()})


@pytest.mark.parametrize("name", ["cosine_5x4x3_k3", "linear_5x4x3_k3", "cosine_37x68x1001_k5", "linear_64x12x129_k5", "cosine_33x256x1_k1"])
def test_cpu_backend_states_what_the_kernels_compute(name):
    """tests/ref_ops_aux_head.py (the kernel header's formulas in fp32) against the float64 restatement, at the GPU tests' bounds:
    plain, with ignored rows, with a zero hidden row and a zero weight row"""
    inp = RA.build_kernel_case(name)
    variants = [(inp, None)]
    if inp["B"] > 3:
        y = inp["y"].clone()
        y[::3] = -100
        variants.append((inp, y))
    if inp["mode"] == "cosine" and inp["C"] > 17:
        z = dict(inp, h=inp["h"].clone(), W=inp["W"].clone())
        z["h"][4] = 0
        z["W"][17] = 0
        variants.append((z, None))
    for case, y in variants:
        ref, got = RA.kernel_reference(case, torch.float64, y=y), _run_cpu_backend(case, y)
        assert abs(got["acc"][0].item() - ref["loss"].item()) <= 5e-5 * abs(ref["loss"].item())
        assert got["acc"][1].item() == ref["top1"].item() and got["acc"][2].item() == ref["topk"].item()
        valid = (case["y"] if y is None else y) != -100
        assert torch.equal(got["rows"][valid, 2].long(), ref["rank"][valid]) and got["acc"][3].item() == valid.sum().item()
        for k in ("dh", "dW", "dlog_scale" if case["mode"] == "cosine" else "dbias"):
            r = ref[k].float()
            assert torch.isfinite(got[k]).all()
            torch.testing.assert_close(got[k], r, rtol=5e-4, atol=1e-7 + 5e-4 * r.abs().max().item(), msg=lambda m: f"{name} {k}: {m}")
    from tests import ref_ops_aux_head as RO

    y = inp["y"].clone()
    y[0] = inp["C"]
    assert torch.isnan(RO.cls_ce_fwd(inp["h"], inp["W"], y, inp["k"], bias=torch.zeros(inp["C"]))[1][0])
    assert torch.isnan(RO.cls_ce_fwd(inp["h"], inp["W"], y * 0 - 100, inp["k"], bias=torch.zeros(inp["C"]))[1][0])
