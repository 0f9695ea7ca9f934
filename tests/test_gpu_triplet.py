"""GPU: the DynaCLR triplet branch — vsx_triplet_fwd / vsx_triplet_bwd behind viscy_amd.contrastive.TripletMarginLoss against
torch.nn.functional on the CPU, and the three-view ContrastiveModule step against three forwards of the oracle encoder.

Bounds.  Op level: those of test_ntxent_general_labels_vs_oracle (the sibling kernel of the same file): loss 5e-5 relative,
gradients rtol 5e-4 / atol 1e-7 + 5e-4 max|grad|.  Model level: those of test_contrastive_encoder_matches_reference_golden_fp32
(1e-3 outputs, 2e-3 per-parameter gradients, running statistics rtol 1e-3 / atol 1e-4) and of
test_graph_captured_contrastive_and_pretraining_steps_match_eager (2e-3 |x| + 1e-5 per step of the trajectory)."""

import functools

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from tests.conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
MARGIN = 0.5
SHAPES = [(2, 4), (5, 1), (7, 3), (37, 63), (37, 64), (37, 65), (64, 128), (600, 128), (5, 1000), (257, 768)]


def make(B, D):
    """a = randn, p = a + r_p u, n = a + r_n v with u, v row-normalised randn and r ~ U[0.5, 2] per row: with margin 0.5 a mix
    of active and inactive rows, none near the kink of its hinge"""
    g = torch.Generator().manual_seed(100 * B + D)
    a = torch.randn(B, D, generator=g)
    u, v = F.normalize(torch.randn(B, D, generator=g), dim=1), F.normalize(torch.randn(B, D, generator=g), dim=1)
    r_p, r_n = 0.5 + 1.5 * torch.rand(B, 1, generator=g), 0.5 + 1.5 * torch.rand(B, 1, generator=g)
    return a, a + r_p * u, a + r_n * v


def torch_reference(a, p, n, margin, reduction):
    """loss, (dA, dP, dN) and the six numbers of `last_stats` from torch on the CPU; the smallest distance to the hinge's kink"""
    a, p, n = (t.clone().requires_grad_(True) for t in (a, p, n))
    loss = nn.TripletMarginLoss(margin=margin, reduction=reduction)(a, p, n)
    loss.backward()
    with torch.no_grad():
        d_ap, d_an = F.pairwise_distance(a, p), F.pairwise_distance(a, n)
        gap = d_ap - d_an + margin
        stats = torch.stack((loss.detach(), F.cosine_similarity(a, p, dim=1).mean(), d_ap.mean(),
                             F.cosine_similarity(a, n, dim=1).mean(), d_an.mean(), (gap > 0).float().mean()))
    return loss.detach(), (a.grad, p.grad, n.grad), stats, gap.abs().min().item()


@functools.lru_cache(maxsize=None)
def reference(B, D, reduction):
    """computed once per case and shared (the determinism test reads the (600, 128) one too); never written to"""
    return make(B, D), torch_reference(*make(B, D), MARGIN, reduction)


def run_gpu(a, p, n, margin, reduction, gout=1.0):
    from viscy_amd.contrastive import TripletMarginLoss

    ag, pg, ng = (t.to(DEV).requires_grad_(True) for t in (a, p, n))
    crit = TripletMarginLoss(margin=margin, reduction=reduction)
    loss = crit(ag, pg, ng)
    (gout * loss).backward()
    return loss.detach().cpu(), (ag.grad.cpu(), pg.grad.cpu(), ng.grad.cpu()), crit.last_stats.cpu()


def check_against(ref, got, what):
    (l_ref, g_ref, s_ref), (l, g, s) = ref, got
    print(what, "loss", l.item(), "ref", l_ref.item(), "stats", s.tolist(), "ref", s_ref.tolist(),
          "max |grad err|", [(x - y).abs().max().item() for x, y in zip(g, g_ref)])
    assert abs(l.item() - l_ref.item()) <= 5e-5 * abs(l_ref.item()), (what, l.item(), l_ref.item())
    for name, x, y in zip(("dA", "dP", "dN"), g, g_ref):
        torch.testing.assert_close(x, y, rtol=5e-4, atol=1e-7 + 5e-4 * y.abs().max().item(), msg=lambda m: f"{what} {name}: {m}")
    assert s.shape == (6,)
    for k in range(6):
        assert abs(s[k].item() - s_ref[k].item()) <= 5e-5 * abs(s_ref[k].item()), (what, k, s[k].item(), s_ref[k].item())


@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("B,D", SHAPES, ids=[f"{b}x{d}" for b, d in SHAPES])
def test_triplet_loss_and_gradients_vs_torch(B, D, reduction):
    """rows per workgroup not dividing B; D below / at / above one wave and no multiple of 4 (scalar path) or one (16-byte
    path); B above one 256-thread sweep of the finalize"""
    (a, p, n), (l_ref, g_ref, s_ref, gap) = reference(B, D, reduction)
    assert gap >= 1e-4, gap   # no row near the kink: both sides agree on which rows are active
    if B >= 7:
        assert 0.5 <= s_ref[5].item() <= 0.9, s_ref[5]   # a mix of active and inactive rows
    check_against((l_ref, g_ref, s_ref), run_gpu(a, p, n, MARGIN, reduction), f"({B}, {D}) {reduction}")


def test_triplet_all_rows_inactive_gives_exact_zeros():
    a, p, n = make(37, 65)
    for reduction in ("mean", "sum"):
        loss, grads, stats = run_gpu(a, p, n, -100.0, reduction)
        assert loss.item() == 0.0 and stats[0].item() == 0.0 and stats[5].item() == 0.0
        for g in grads:
            assert torch.equal(g, torch.zeros_like(g))


def test_triplet_zero_distance_row_and_identical_positive():
    """row 0: a = 0, p = 1e-6 = eps, so a - p + eps and d_ap are exactly 0: that term contributes no gradient (torch's norm
    backward), dA = -dN.  Row 1: p == a, d_ap = eps sqrt(D).  Row 2: an ordinary row."""
    from viscy_amd import ops

    D = 4
    a, p, n = make(3, D)
    a[0], p[0], n[0] = 0.0, 1e-6, 1.0
    p[1] = a[1]
    ref = torch_reference(a, p, n, 5.0, "mean")
    assert ref[3] >= 1e-4
    got = run_gpu(a, p, n, 5.0, "mean")
    rows, _ = ops.triplet_fwd(a.to(DEV), p.to(DEV), n.to(DEV), 5.0, 1e-6, "mean")
    rows = rows.cpu()
    assert rows[0, 0].item() == 0.0 and F.pairwise_distance(a, p)[0].item() == 0.0
    assert abs(rows[1, 0].item() - 1e-6 * D ** 0.5) <= 5e-5 * 1e-6 * D ** 0.5
    assert (rows[:, 2] > 0).all()   # margin 5: every row is active
    for t in (got[0], *got[1], got[2], rows):
        assert torch.isfinite(t).all()
    dA, dP, dN = got[1]
    assert torch.equal(dP[0], torch.zeros(D)) and torch.equal(dA[0], -dN[0]) and dN[0].abs().min() > 0
    check_against(ref[:3], got, "exact rows")


def test_triplet_is_bit_identical_from_run_to_run():
    from viscy_amd import ops

    (a, p, n), _ = reference(600, 128, "mean")
    runs = []
    for _ in range(2):
        loss, grads, stats = run_gpu(a, p, n, MARGIN, "mean", gout=1.7)
        rows, acc = ops.triplet_fwd(a.to(DEV), p.to(DEV), n.to(DEV), MARGIN, 1e-6, "mean")
        runs.append((loss, *grads, stats, rows.cpu(), acc.cpu()))
    assert torch.equal(runs[0][-1], runs[0][4])   # last_stats is the kernel's acc
    for x, y in zip(*runs):
        assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------ model level
def relerr(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


# parameters whose exact gradient is zero here, so that both sides hold round-off only (the oracle: <= 4e-7 next to >= 7e-3
# for every other parameter).  The first three are shifts constant over the batch in front of a train-mode BatchNorm, and
# nothing else reads the embedding (tests/test_schedule_cpu.py makes the same exception).  projection.4.bias shifts the
# projections of all three views alike, and the triplet loss reads only their differences: sum_i (dA_i + dP_i + dN_i) = 0.
ZERO_GRAD = ("projection.0.bias", "projection.3.bias", "encoder.head.norm.bias", "projection.4.bias")


def _triplet_views(g):
    x = torch.randn(g["x_shape"], generator=torch.Generator().manual_seed(g["x_seed"]))
    gen = torch.Generator().manual_seed(5)
    # two noisy copies of the anchor: the CPU side finds three rows of four active, none within 0.2 of the hinge's kink
    return x, x + 0.5 * torch.randn(x.shape, generator=gen), x + 0.5 * torch.randn(x.shape, generator=gen)


@functools.lru_cache(maxsize=None)
def _oracle_triplet_step():
    """three separate train-mode forwards of the oracle encoder and torch's TripletMarginLoss(0.5), on the CPU, once"""
    from oracle import contrastive_ref as C

    g = load_golden("contrastive.pt")["v2_small_z9"]
    ref = C.randomize_encoder_(C.ContrastiveEncoder(**g["kwargs"], **g["arch"]), seed=g["seed"]).train()
    start = {k: v.clone() for k, v in ref.state_dict().items()}
    proj = [ref(v)[1] for v in _triplet_views(g)]
    loss = nn.TripletMarginLoss(margin=MARGIN)(*proj)
    loss.backward()
    with torch.no_grad():
        gap = F.pairwise_distance(proj[0], proj[1]) - F.pairwise_distance(proj[0], proj[2]) + MARGIN
    grads = {k: p.grad.clone() for k, p in ref.named_parameters()}
    after = {k: v.clone() for k, v in ref.state_dict().items() if "running" in k or "num_batches" in k}
    return g, start, loss.detach(), grads, after, gap


@pytest.mark.parametrize("paired", [True, False], ids=["one_pass", "three_forwards"])
def test_triplet_step_matches_three_oracle_forwards_fp32(paired):
    from viscy_amd.contrastive import ContrastiveEncoder, ContrastiveModule

    g, start, l_ref, g_ref, after, gap = _oracle_triplet_step()
    # active and inactive rows, none near the kink (the projections carry up to 1e-3 of relative error)
    assert gap.abs().min() >= 0.1 and (gap > 0).any() and (gap < 0).any() and l_ref.item() > 0.1, gap
    enc = ContrastiveEncoder(**g["kwargs"], **g["arch"])
    enc.load_state_dict(start, strict=True)
    mod = ContrastiveModule(enc, loss_function=nn.TripletMarginLoss(margin=MARGIN)).cuda().train()
    enc.compute_dtype = torch.float32
    mod.paired_forward = paired
    a, p, n = (v.cuda() for v in _triplet_views(g))
    loss = mod.training_step({"anchor": a, "positive": p, "negative": n}, 0)
    loss.backward()
    print("triplet step", "paired" if paired else "separate", "loss", loss.item(), "ref", l_ref.item())
    assert relerr(loss, l_ref) <= 1e-3
    worst = 0.0
    for name, prm in enc.named_parameters():
        if name in ZERO_GRAD:
            assert prm.grad.abs().max() < 1e-4 and g_ref[name].abs().max() < 1e-4, name
            continue
        e = relerr(prm.grad, g_ref[name])
        worst = max(worst, e)
        assert e <= 2e-3, (name, e)
    print("worst relative gradient error", worst)
    sd = enc.state_dict()
    assert len(after) == 6
    for k, v in after.items():
        if "num_batches" in k:
            assert int(sd[k]) == int(v) == 3, k   # one update per view
        else:
            torch.testing.assert_close(sd[k].cpu().float(), v.float(), rtol=1e-3, atol=1e-4)


def test_graph_captured_triplet_step_matches_eager_and_logs_nothing():
    from viscy_amd.contrastive import ContrastiveEncoder, ContrastiveModule

    g = torch.Generator().manual_seed(1)
    a = torch.randn(4, 1, 5, 64, 64, generator=g).cuda()
    p = a + 0.3 * torch.randn(a.shape, generator=g).cuda()
    n = torch.randn(a.shape, generator=g).cuda()
    keys = ["metrics/cosine_similarity/positive/{}", "metrics/euclidean_distance/positive/{}",
            "metrics/cosine_similarity_negative/{}", "metrics/euclidean_distance_negative/{}"]
    traj = []
    for use_graph in (False, True):
        torch.manual_seed(0)
        enc = ContrastiveEncoder("convnext_tiny", in_channels=1, in_stack_depth=5, embedding_dim=64, projection_dim=32,
                                 depths=(1, 1, 2, 1), dims=(32, 64, 96, 128))
        mod = ContrastiveModule(enc, loss_function=nn.TripletMarginLoss(margin=MARGIN), lr=1e-3).cuda()
        enc.compute_dtype = torch.float32
        opt = mod.configure_optimizers(t_total=8)
        mod.train()
        step = mod.make_train_step(opt, use_graph=use_graph)
        traj.append([step(a, p, n).item() for _ in range(8 if not use_graph else 6)])
        # three forwards per step; the capture's warm-up steps are undone
        assert int(enc.projection[1].num_batches_tracked) == (24 if not use_graph else 18)
        assert not mod.logged   # a train step keeps nothing: captured tensors must not pile up in the log
    assert all(abs(x - y) <= 2e-3 * abs(x) + 1e-5 for x, y in zip(traj[0][:6], traj[1])), traj
    # an eager training_step / validation_step logs the loss and the reference's four metrics (engine.py:135-146)
    loss = mod.training_step({"anchor": a, "positive": p, "negative": n}, 0)
    mod.eval()
    with torch.no_grad():
        mod.validation_step({"anchor": a, "positive": p, "negative": n}, 0)
    for stage in ("train", "val"):
        assert sorted(k for k in mod.logged if k.endswith("/" + stage)) == sorted([f"loss/{stage}"] + [k.format(stage) for k in keys])
    stats = mod.loss_function.last_stats
    assert float(mod.logged["loss/train"][0]) == loss.item()
    assert float(mod.logged["metrics/euclidean_distance_negative/val"][0]) == stats[4].item()
    assert -1.0 <= float(mod.logged["metrics/cosine_similarity/positive/train"][0]) <= 1.0
