"""GPU: the DynaCLR auxiliary ClassificationHead — vsx_cls_ce_fwd / vsx_cls_ce_bwd / vsx_cls_logits against the float64
restatement of tests/ref_aux_heads.py (pinned to the reference by tests/golden/aux_heads.pt), viscy_amd.heads.ClassificationHead
against the reference's recorded head cases, and the ContrastiveModule step with a head against the oracle composition.

Bounds.  Op and head level: those of tests/test_gpu_triplet.py — loss 5e-5 relative, gradients rtol 5e-4 / atol 1e-7 +
5e-4 max|ref|; torch in fp32 alone stays within 1.3e-5 (loss) and 3e-5 of the largest entry (gradients) on these shapes.
Accuracies: every label sits at >= 1e-3 from every other logit of its row (asserted where the cases are built), fp32 logits
carry <= ~1e-5, so top-1 / top-k equal the float64 counts exactly.  Model level: those of the triplet step test (1e-3 loss and
logged values, 2e-3 per-parameter gradients)."""

import functools
import math

import pytest
import torch
import torch.nn.functional as F

from tests import ref_aux_heads as RA
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"


@functools.lru_cache(maxsize=None)
def reference(name):
    """the case's inputs and its float64 restatement, computed once and shared; never written to"""
    inp = RA.build_kernel_case(name)
    return inp, RA.kernel_reference(inp, torch.float64)


def run_gpu(inp, y=None, splits=0, gout=RA.GOUT):
    """forward + backward of the kernels on the case's tensors -> dict of CPU tensors (rows, acc, dh, dW, dbias | dlog_scale)"""
    from viscy_amd import ops

    h, W = inp["h"].to(DEV), inp["W"].to(DEV)
    y = (inp["y"] if y is None else y).to(DEV)
    cls, grads = {}, {}
    if "log_scale" in inp:
        cls = dict(inv_h=ops.cls_inv_norm(h), inv_w=ops.cls_inv_norm(W), log_scale=inp["log_scale"].to(DEV).view(1))
        grads = dict(dlog_scale=torch.zeros(1, device=DEV))
    else:
        cls = dict(bias=inp["bias"].to(DEV))
        grads = dict(dbias=torch.zeros(W.shape[0], device=DEV))
    rows, acc = ops.cls_ce_fwd(h, W, y, inp["k"], splits=splits, **cls)
    dW = torch.zeros_like(W)
    dh = ops.cls_ce_bwd(h, W, y, rows, acc, torch.tensor([gout], device=DEV), dW, **cls, **grads)
    out = dict(rows=rows.cpu(), acc=acc.cpu(), dh=dh.cpu(), dW=dW.cpu(), logits=ops.cls_logits(h, W, **cls).cpu())
    out.update({k: v.cpu().reshape(inp[k[1:]].shape) for k, v in grads.items()})
    return out


def check_grads(got, ref, keys, what):
    for k in keys:
        r = ref[k].float()
        print(what, k, "max |err|", (got[k] - r).abs().max().item(), "max |ref|", r.abs().max().item())
        torch.testing.assert_close(got[k], r, rtol=5e-4, atol=1e-7 + 5e-4 * r.abs().max().item(), msg=lambda m: f"{what} {k}: {m}")


# ------------------------------------------------------------------------------------------------ kernels against float64
@pytest.mark.parametrize("name", list(RA.KERNEL_CASES))
def test_kernels_match_the_float64_restatement(name):
    inp, ref = reference(name)
    got = run_gpu(inp)
    loss, top1, topk, n = got["acc"].tolist()
    print(name, "loss", loss, "ref", ref["loss"].item(), "top1", top1, "topk", topk, "ref", ref["top1"].item(), ref["topk"].item())
    assert abs(loss - ref["loss"].item()) <= 5e-5 * abs(ref["loss"].item())
    assert top1 == ref["top1"].item() and topk == ref["topk"].item() and n == inp["B"]
    assert torch.equal(got["rows"][:, 2].long(), ref["rank"]) and (got["rows"][:, 3] == 1).all()
    lse64 = torch.logsumexp(ref["logits"], 1)
    torch.testing.assert_close(got["rows"][:, 0].double(), lse64, rtol=1e-5, atol=1e-5)
    zy64 = ref["logits"].gather(1, inp["y"][:, None])[:, 0]
    torch.testing.assert_close(got["rows"][:, 1].double(), zy64, rtol=1e-5, atol=1e-5)
    # the materialised logits are the ones the fused path ranks: the target's is bit-identical
    assert torch.equal(got["logits"].gather(1, inp["y"][:, None])[:, 0], got["rows"][:, 1])
    torch.testing.assert_close(got["logits"].double(), ref["logits"], rtol=1e-5, atol=1e-5)
    check_grads(got, ref, ("dh", "dW", "dlog_scale" if inp["mode"] == "cosine" else "dbias"), name)


# ------------------------------------------------------------------------------------------------ exact ties
def _tie_case():
    """linear head on integers (dots exact in fp32).  Classes c and c + 150 share their weight row and bias, so they tie in every
    row; even rows take the upper twin as target (its twin sits at a LOWER index, one class tile away), odd rows the lower
    one (twin at a HIGHER index).  C = 300: three class tiles, so a tie also crosses tile and split boundaries."""
    g = torch.Generator().manual_seed(5)
    B, H, C = 70, 8, 300
    h = torch.randint(-3, 4, (B, H), generator=g).float()
    W = torch.randint(-3, 4, (C, H), generator=g).float()
    bias = torch.randint(-2, 3, (C,), generator=g).float()
    W[150:], bias[150:] = W[:150], bias[:150]
    base = torch.randint(0, 150, (B,), generator=g)
    even = torch.arange(B) % 2 == 0
    y = torch.where(even, base + 150, base)
    return dict(mode="linear", h=h, W=W, bias=bias, y=y, k=3, B=B), even


def test_exact_ties_follow_the_total_order_for_every_split_count():
    inp, even = _tie_case()
    Z = inp["h"].double() @ inp["W"].double().t() + inp["bias"].double()
    assert torch.equal((inp["h"] @ inp["W"].t() + inp["bias"]).double(), Z)   # exact in fp32: integers
    zy = Z.gather(1, inp["y"][:, None])
    rank, strictly, ties = RA.rank_of_target(Z, inp["y"]), (Z > zy).sum(1), (Z == zy).sum(1) - 1
    assert (ties >= 1).all()
    assert (rank[even] >= strictly[even] + 1).all()          # the twin at the lower index is ahead of the target ...
    assert (rank[~even] <= strictly[~even] + ties[~even] - 1).all()   # ... the twin at the higher index is not
    runs = [run_gpu(inp, splits=s) for s in (0, 1, 2, 3)]
    assert torch.equal(runs[0]["rows"][:, 2].long(), rank)
    assert torch.equal(runs[0]["logits"].double(), Z)
    B = inp["B"]
    assert runs[0]["acc"][1].item() == ((rank == 0).sum() / B).item() and runs[0]["acc"][2].item() == ((rank < 3).sum() / B).item()
    for r in runs[1:]:
        for k in ("rows", "acc", "dh", "dW", "dbias"):
            assert torch.equal(r[k], runs[0][k]), k


def test_split_count_does_not_change_a_bit_on_float_inputs():
    name = "cosine_130x256x1001_k5"
    inp, _ = reference(name)
    runs = [run_gpu(inp, splits=s) for s in (0, 1, 3, 8)]
    for r in runs[1:]:
        assert torch.equal(r["rows"], runs[0]["rows"]) and torch.equal(r["acc"], runs[0]["acc"])


# ------------------------------------------------------------------------------------------------ labels
@pytest.mark.parametrize("name", ["cosine_37x68x1001_k5", "linear_64x12x129_k5"])
def test_ignored_rows_count_in_no_sum_and_get_exact_zero_gradients(name):
    inp, _ = reference(name)
    y = inp["y"].clone()
    y[::3] = -100
    ref = RA.kernel_reference(inp, torch.float64, y=y)
    got = run_gpu(inp, y=y)
    loss, top1, topk, n = got["acc"].tolist()
    assert n == (y != -100).sum().item() and abs(loss - ref["loss"].item()) <= 5e-5 * abs(ref["loss"].item())
    assert top1 == ref["top1"].item() and topk == ref["topk"].item()
    assert (got["rows"][::3, 3] == 0).all() and (got["dh"][::3] == 0).all() and (got["dh"][1::3].abs().sum(1) > 0).all()
    check_grads(got, ref, ("dh", "dW", "dlog_scale" if inp["mode"] == "cosine" else "dbias"), name + " ignore mix")
    # all ignored: NaN, as torch gives
    y[:] = -100
    got = run_gpu(inp, y=y)
    assert math.isnan(got["acc"][0].item()) and got["acc"][3].item() == 0 and math.isnan(F.cross_entropy(inp["h"][:, :3], y).item())
    assert (got["dh"] == 0).all() and (got["dW"] == 0).all()


@pytest.mark.parametrize("bad", [1001, -1, 2 ** 40, -(2 ** 40)])
def test_labels_outside_the_classes_give_nan_and_index_nothing(bad):
    inp, _ = reference("cosine_37x68x1001_k5")
    y = inp["y"].clone()
    y[5] = bad
    got = run_gpu(inp, y=y)
    assert math.isnan(got["acc"][0].item()) and got["rows"][5, 3].item() == -1 and got["acc"][3].item() == inp["B"] - 1


# ------------------------------------------------------------------------------------------------ zero rows, non-finite logits
def test_zero_hidden_row_and_zero_weight_row_have_finite_gradients_as_torch():
    inp, _ = reference("cosine_37x68x1001_k5")
    inp = dict(inp, h=inp["h"].clone(), W=inp["W"].clone())
    inp["h"][4] = 0
    inp["W"][17] = 0
    ref = RA.kernel_reference(inp, torch.float64)
    got = run_gpu(inp)
    assert all(torch.isfinite(got[k]).all() for k in ("dh", "dW", "dlog_scale", "rows", "acc"))
    assert (got["logits"][4] == 0).all() and (got["logits"][:, 17] == 0).all()
    assert abs(got["acc"][0].item() - ref["loss"].item()) <= 5e-5 * abs(ref["loss"].item())
    assert got["dh"][4].abs().max() > 1e6 and got["dW"][17].abs().max() > 1e6   # 1 / eps = 1e12 times the direction's gradient
    check_grads(got, ref, ("dh", "dW", "dlog_scale"), "zero rows")
    # next to the 1e12-sized rows the bound above says little about the others: those once more on their own
    keep_h = torch.arange(inp["B"]) != 4
    keep_w = torch.arange(1001) != 17
    check_grads(dict(dh=got["dh"][keep_h], dW=got["dW"][keep_w]), dict(dh=ref["dh"][keep_h], dW=ref["dW"][keep_w]), ("dh", "dW"),
                "zero rows, the others")


def test_non_finite_logits_reach_the_loss_as_in_torch():
    inp, _ = reference("linear_64x12x129_k5")
    for value in (float("nan"), float("inf")):
        bias = inp["bias"].clone()
        bias[100] = value
        got = run_gpu(dict(inp, bias=bias))
        ref = F.cross_entropy(inp["h"] @ inp["W"].t() + bias, inp["y"])
        assert math.isnan(ref.item()) and math.isnan(got["acc"][0].item()), value


# ------------------------------------------------------------------------------------------------ determinism
def test_forward_and_backward_are_bit_identical_from_run_to_run():
    for name in ("cosine_130x256x1001_k5", "linear_257x32x64_k5"):
        inp, _ = reference(name)
        a, b = run_gpu(inp, gout=1.7), run_gpu(inp, gout=1.7)
        for k in a:   # the header promises every gradient, not only the forward
            assert torch.equal(a[k], b[k]), (name, k)


# ------------------------------------------------------------------------------------------------ the head module
@pytest.mark.parametrize("name", list(RA.HEAD_CASES))
def test_head_module_matches_the_reference_record(name):
    from viscy_amd.heads import ClassificationHead

    gold = load_golden("aux_heads.pt")["head"][name]["fp64"]
    case = RA.build_head_case(name)
    head = ClassificationHead(**RA.HEAD_CASES[name]["kwargs"])
    head.load_state_dict(case["head"].state_dict(), strict=True)
    head = head.to(DEV).train()
    x = case["x"].to(DEV).requires_grad_(True)
    loss, stats = head.loss_and_stats(x, case["y"].to(DEV))
    (loss * RA.GOUT).backward()
    pick = lambda t: t.detach().cpu().reshape(-1)[RA.grad_sample_index(t.numel())]  # noqa: E731
    hn, k = head.head_name, head.top_k
    print(name, "loss", loss.item(), "ref", gold["loss"])
    assert abs(loss.item() - gold["loss"]) <= 5e-5 * abs(gold["loss"])
    assert stats["top1"].item() == gold["logged"][f"metrics/acc_top1/{hn}/train"]
    assert stats["topk"].item() == gold["logged"][f"metrics/acc_top{k}/{hn}/train"] and stats["n_valid"].item() == x.shape[0]
    got = {"dx": pick(x.grad), **{n: pick(p.grad) for n, p in head.named_parameters()}}
    ref = {"dx": gold["dx"], **gold["grads"]}
    check_grads(got, ref, list(ref), name)
    for n, b in head.named_buffers():
        torch.testing.assert_close(pick(b).double(), gold["buffers"][n].double(), rtol=1e-5, atol=1e-6, msg=lambda m: f"{name} {n}: {m}")
    # inference: running statistics, materialised logits, no autograd history; the restated head in eval mode is the reference
    head.eval()
    ref_head = case["head"]
    ref_head.load_state_dict({k: v.cpu() for k, v in head.state_dict().items()})
    with torch.no_grad():
        want = ref_head.double().eval()(case["x"].double())
    logits = head(case["x"].to(DEV))
    assert not logits.requires_grad
    torch.testing.assert_close(logits.cpu().double(), want, rtol=1e-4, atol=1e-4)
    with pytest.raises(RuntimeError, match="gradient"):
        head(x)
    with torch.no_grad():
        l_eval, _ = head.loss_and_stats(case["x"].to(DEV), case["y"].to(DEV))
    assert abs(l_eval.item() - F.cross_entropy(want, case["y"]).item()) <= 5e-5 * l_eval.item()


# ------------------------------------------------------------------------------------------------ module level
def relerr(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


# exact gradient zero, so that both sides hold round-off only: shifts constant over the batch in front of a train-mode BatchNorm
# (the head's first layer is Linear -> BatchNorm1d too, so encoder.head.norm.bias, which shifts every embedding alike, stays
# in this list with a head attached); the triplet loss reads differences of projections only.  tests/test_gpu_triplet.py
# makes the same exceptions.
ZERO_GRAD = {"ntxent": ("projection.0.bias", "projection.3.bias", "encoder.head.norm.bias"),
             "triplet": ("projection.0.bias", "projection.3.bias", "encoder.head.norm.bias", "projection.4.bias")}
HEAD_ZERO_GRAD = ("mlp.backbone.0.bias",)


@functools.lru_cache(maxsize=None)
def oracle_step(kind):
    return RA.oracle_module_step(kind)


@pytest.mark.parametrize("kind", ["ntxent", "triplet"])
def test_module_step_with_a_head_matches_the_oracle_composition(kind):
    from torch import nn

    from viscy_amd.contrastive import ContrastiveEncoder, ContrastiveModule, NTXentLoss
    from viscy_amd.heads import ClassificationHead

    o = oracle_step(kind)
    assert o["label_gap"] >= 0.05
    enc = ContrastiveEncoder("convnextv2_tiny", in_channels=1, in_stack_depth=5, **RA.SMALL)
    enc.load_state_dict(o["start"]["enc"], strict=True)
    head = ClassificationHead(**RA.MODULE_HEAD)
    head.load_state_dict(o["start"]["head"], strict=True)
    loss_fn = NTXentLoss(temperature=RA.TEMPERATURE) if kind == "ntxent" else nn.TripletMarginLoss(margin=RA.MARGIN)
    mod = ContrastiveModule(enc, loss_function=loss_fn, lr=RA.MODULE_LR, example_input_array_shape=(1, 1, 5, 32, 32),
                            auxiliary_heads={"gene": head}).cuda().train()
    enc.compute_dtype = torch.float32
    opt = mod.configure_optimizers()
    batch = {k: v.cuda() for k, v in o["batch"].items() if kind == "triplet" or k != "negative"}
    opt.zero_grad()
    loss = mod.training_step(batch, 0)
    loss.backward()
    print(kind, "loss", loss.item(), "ref", o["total"].item())
    assert relerr(loss, o["total"]) <= 1e-3
    assert sorted(mod.logged) == sorted(o["logged"])
    for k, v in o["logged"].items():
        got = float(mod.logged[k][0])
        assert got == float(v) if "acc_top" in k else abs(got - float(v)) <= 1e-3 * abs(float(v)), (k, got, float(v))
    worst = 0.0
    for group, module, zero in (("enc", enc, ZERO_GRAD[kind]), ("head", head, HEAD_ZERO_GRAD)):
        for name, prm in module.named_parameters():
            ref = o["grads"][group][name]
            assert prm.grad is not None and prm.grad.data_ptr() == module.engine().g(prm).data_ptr(), name   # flat mode
            if name in zero:
                assert prm.grad.abs().max() < 1e-4 and ref.abs().max() < 1e-4, name
                continue
            e = relerr(prm.grad, ref)
            worst = max(worst, e)
            assert e <= 2e-3, (group, name, e)
    print("worst relative gradient error", worst)
    # one optimiser object, one step count: the head's parameters move as torch.optim.AdamW moves them on the same gradients
    before = {n: p.detach().cpu().clone() for n, p in head.named_parameters()}
    grads = {n: p.grad.detach().cpu().clone() for n, p in head.named_parameters()}
    stem_before = enc.stem.conv.weight.detach().clone()
    opt.step()
    assert opt.t == 1 and int(opt.step_dev) == 1 and not torch.equal(stem_before, enc.stem.conv.weight)
    twins = [nn.Parameter(before[n].clone()) for n in before]
    for t, n in zip(twins, before):
        t.grad = grads[n]
    torch.optim.AdamW(twins, lr=RA.MODULE_LR).step()
    for t, (n, p) in zip(twins, head.named_parameters()):
        torch.testing.assert_close(p.detach().cpu(), t.detach(), rtol=1e-5, atol=1e-7, msg=lambda m: f"{n} after AdamW: {m}")
        if n not in HEAD_ZERO_GRAD:   # and, away from |g| ~ eps, as the oracle's own step moved them
            big = o["grads"]["head"][n].abs() > 1e-3 * o["grads"]["head"][n].abs().max()
            torch.testing.assert_close(p.detach().cpu()[big], o["head_after"][n][big], rtol=1e-4, atol=2e-2 * RA.MODULE_LR)


class _Batches:
    """a list-of-batches datamodule; labels ride in ``anchor_meta`` as a TripletDataModule hands them over"""
    training = True

    def __init__(self):
        g = torch.Generator().manual_seed(3)
        a = torch.randn(4, 1, 5, 32, 32, generator=g)
        meta = [{"labels": {"gene_label": r % 7}} for r in range(4)]
        self.batch = {"anchor": a, "positive": a + 0.3 * torch.randn(a.shape, generator=g), "anchor_meta": meta}

    def prepare_data(self):
        pass

    def setup(self, stage):
        pass

    def train_dataloader(self):
        return [self.batch]

    def val_dataloader(self):
        return [self.batch]

    def on_after_batch_transfer(self, batch, dataloader_idx):
        return batch


def test_two_epoch_fit_steps_and_logs_the_loss_weight():
    from viscy_amd.contrastive import ContrastiveEncoder, ContrastiveModule
    from viscy_amd.heads import ClassificationHead
    from viscy_amd.trainer import Trainer

    torch.manual_seed(0)
    enc = ContrastiveEncoder("convnextv2_tiny", in_channels=1, in_stack_depth=5, **RA.SMALL)
    head = ClassificationHead(**dict(RA.MODULE_HEAD, weight_schedule="cosine", weight_start=0.0, weight_warmup_epochs=2))
    mod = ContrastiveModule(enc, lr=1e-3, example_input_array_shape=(1, 1, 5, 32, 32), auxiliary_heads={"gene": head})
    enc.compute_dtype = torch.float32
    w0 = head.mlp.head.weight.detach().clone()
    Trainer(max_epochs=2, precision="32-true", seed=0).fit(mod, _Batches())
    assert mod.logged["hparams/loss_weight/gene"] == [RA.cosine_anneal(0.0, 0.5, 0, 2), RA.cosine_anneal(0.0, 0.5, 1, 2)] == [0.0, pytest.approx(0.25, rel=1e-12)]
    for stage in ("train", "val"):
        for key in (f"loss/aux/gene/{stage}", f"metrics/acc_top1/gene/{stage}", f"metrics/acc_top3/gene/{stage}"):
            assert len(mod.logged[key]) == 2 and all(torch.isfinite(v) for v in mod.logged[key]), key
    # epoch 0 trains the head with weight 0 (weight decay alone), epoch 1 with 0.25: it has moved
    assert not torch.equal(w0.to(head.mlp.head.weight.device), head.mlp.head.weight.detach())
    assert int(head.mlp.backbone[1].num_batches_tracked) == 2
