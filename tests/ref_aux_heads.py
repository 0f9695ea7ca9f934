"""TEST INFRASTRUCTURE — a plain-torch, float64-capable restatement of the embedding-space heads that viscy_amd.heads builds
(``viscy_models.components.heads``: ``CosineClassifier``, ``MLP`` in classification mode, ``ClassificationHead.compute_loss`` /
``log_metrics``, ``BaseHead.step``), pinned against the reference by tests/golden/aux_heads.pt
(tools/gen_golden_aux_heads.py), and the case tables of the head tests.  Inputs are never stored: seeds and shapes rebuild
them.  Modules are constructed in the reference's order, so that the same ``torch.manual_seed`` gives the same parameters."""

from __future__ import annotations

import math

import torch
import torch.nn.functional as F
from torch import nn

# ------------------------------------------------------------------------------------------------ the restatement
class CosineClassifier(nn.Module):
    def __init__(self, in_dim, num_classes, init_scale=20.0, learn_scale=True):
        super().__init__()
        self.weight = nn.Parameter(torch.randn(num_classes, in_dim))
        nn.init.normal_(self.weight, std=0.01)
        scale = torch.tensor(math.log(init_scale))
        if learn_scale:
            self.log_scale = nn.Parameter(scale)
        else:
            self.register_buffer("log_scale", scale)

    def forward(self, x):
        return self.log_scale.exp() * (F.normalize(x, dim=1) @ F.normalize(self.weight, dim=1).t())


class MLP(nn.Module):
    """classification mode: (Linear -> BatchNorm1d -> ReLU) per hidden width, then the classifier"""

    def __init__(self, in_dims, hidden_dims, num_classes, cosine_classifier=True):
        super().__init__()
        widths = [hidden_dims] if isinstance(hidden_dims, int) else list(hidden_dims)
        layers, prev = [], in_dims
        for w in widths:
            layers += [nn.Linear(prev, w), nn.BatchNorm1d(w), nn.ReLU(inplace=True)]
            prev = w
        self.backbone = nn.Sequential(*layers)
        self.head = CosineClassifier(prev, num_classes) if cosine_classifier else nn.Linear(prev, num_classes)

    def forward(self, x):
        return self.head(self.backbone(x))


def cosine_anneal(start, end, epoch, warmup_epochs):
    if epoch >= warmup_epochs:
        return end
    return end + (start - end) * 0.5 * (1.0 + math.cos(math.pi * epoch / warmup_epochs))


class ClassificationHead(nn.Module):
    def __init__(self, head_name, batch_key, in_dims, hidden_dims, num_classes, cosine_classifier=True, loss_weight=1.0, top_k=5,
                 weight_schedule="constant", weight_start=0.0, weight_warmup_epochs=50):
        super().__init__()
        self.head_name, self.batch_key, self.top_k = head_name, batch_key, top_k
        self.loss_weight, self.weight_schedule = loss_weight, weight_schedule
        self.weight_start, self.weight_warmup_epochs = weight_start, weight_warmup_epochs
        self._current_weight = weight_start if weight_schedule == "cosine" else loss_weight
        self.mlp = MLP(in_dims, hidden_dims, num_classes, cosine_classifier)

    def step(self, epoch):
        if self.weight_schedule == "cosine":
            self._current_weight = cosine_anneal(self.weight_start, self.loss_weight, epoch, self.weight_warmup_epochs)

    def get_weight(self):
        return self._current_weight

    def forward(self, x):
        return self.mlp(x)

    def compute_loss(self, logits, y):
        return F.cross_entropy(logits, y)

    def log_metrics(self, out, log_fn, stage):
        top1, topk = accuracies(out["logits"], out["y"], self.top_k)
        log_fn(f"loss/aux/{self.head_name}/{stage}", out["loss"])
        log_fn(f"metrics/acc_top1/{self.head_name}/{stage}", top1)
        log_fn(f"metrics/acc_top{self.top_k}/{self.head_name}/{stage}", topk)


def accuracies(logits, y, k):
    top1 = (logits.argmax(dim=1) == y).float().mean()
    topk = (logits.topk(k, dim=1).indices == y.unsqueeze(1)).any(dim=1).float().mean()
    return top1, topk


def rank_of_target(logits, y):
    """number of classes ahead of the target in the total order (logit descending, class ascending)"""
    zy = logits.gather(1, y[:, None])
    idx = torch.arange(logits.shape[1])[None]
    return ((logits > zy) | ((logits == zy) & (idx < y[:, None]))).sum(1)


def classifier_logits(h, W, *, log_scale=None, bias=None):
    """the two classifiers as functions of their tensors, in the dtype of ``h``"""
    if log_scale is not None:
        return log_scale.exp() * (F.normalize(h, dim=1) @ F.normalize(W, dim=1).t())
    return h @ W.t() + bias


# ------------------------------------------------------------------------------------------------ kernel cases
LABEL_MARGIN = 1e-3   # every label's logit is at least this far from every other logit of its row
GOUT = 0.7

KERNEL_SHAPES = ((1, 4, 2, 1), (5, 4, 3, 3), (64, 12, 127, 5), (64, 12, 128, 5), (64, 12, 129, 5), (257, 32, 64, 5),
                 (37, 68, 1001, 5), (130, 256, 1001, 5), (33, 256, 1, 1))
KERNEL_CASES = {f"{mode}_{B}x{H}x{C}_k{k}": dict(mode=mode, B=B, H=H, C=C, k=k, seed=100 + 7 * i + (mode == "linear"))
                for i, (B, H, C, k) in enumerate(KERNEL_SHAPES) for mode in ("cosine", "linear")}


def build_kernel_case(name: str) -> dict:
    """h, W, (log_scale | bias), labels, k of a kernel case: even rows take a class from the float64 top-k, odd rows any class,
    each moved on (cyclically) to the next class that keeps LABEL_MARGIN; asserted here"""
    c = KERNEL_CASES[name]
    B, H, C, k = c["B"], c["H"], c["C"], c["k"]
    g = torch.Generator().manual_seed(c["seed"])
    h = torch.randn(B, H, generator=g)
    if c["mode"] == "cosine":
        W = torch.randn(C, H, generator=g) * 0.01
        # the initial temperature; scale 1 for the tiny class counts, where logits 20 apart would put a one-row loss (e^-40)
        # below what lse - z_y resolves in fp32 at ANY accuracy of the parts
        extra = dict(log_scale=torch.tensor(math.log(20.0) if C >= 16 else 0.0))
    else:
        W = torch.randn(C, H, generator=g) / math.sqrt(H)
        extra = dict(bias=torch.randn(C, generator=g) * 0.1)
    Z = classifier_logits(h.double(), W.double(), **{n: v.double() for n, v in extra.items()})
    order = Z.argsort(dim=1, descending=True)
    start = torch.randint(0, C, (B,), generator=g)
    y = torch.empty(B, dtype=torch.long)
    for b in range(B):
        first = int(order[b, (b // 2) % k]) if b % 2 == 0 else int(start[b])
        cands = [int(j) for j in order[b, :k]] if b % 2 == 0 else [(first + s) % C for s in range(C)]
        cands = cands[cands.index(first):] + cands[: cands.index(first)]
        for j in cands:
            gap = (Z[b] - Z[b, j]).abs()
            gap[j] = float("inf")
            if C == 1 or gap.min() >= LABEL_MARGIN:
                y[b] = j
                break
        else:
            raise AssertionError(f"{name}: row {b} has no class with a margin of {LABEL_MARGIN}")
    gap = (Z - Z.gather(1, y[:, None])).abs().scatter(1, y[:, None], float("inf"))
    assert C == 1 or float(gap.min()) >= LABEL_MARGIN, name
    return dict(c, h=h, W=W, y=y, **extra)


def kernel_reference(inp: dict, dtype=torch.float64, y=None) -> dict:
    """loss, top-1, top-k (the reference's .float().mean()), the ranks, and the gradients times GOUT, in ``dtype``"""
    y = inp["y"] if y is None else y
    leaves = {n: inp[n].to(dtype).clone().requires_grad_(True) for n in ("h", "W", "log_scale", "bias") if n in inp}
    Z = classifier_logits(leaves["h"], leaves["W"], **{n: v for n, v in leaves.items() if n in ("log_scale", "bias")})
    loss = F.cross_entropy(Z, y)
    (loss * GOUT).backward()
    valid = y != -100
    ys = y.clamp_min(0)
    rank = rank_of_target(Z.detach(), ys)
    B = Z.shape[0]
    out = dict(loss=loss.detach(), logits=Z.detach(), rank=rank,
               top1=((rank == 0) & valid).sum().float() / B, topk=((rank < inp["k"]) & valid).sum().float() / B)
    out.update({"d" + n: v.grad for n, v in leaves.items()})
    return out


def grad_sample_index(n: int, cap: int = 32) -> torch.Tensor:
    """every entry of a small gradient, ``cap`` evenly spread ones of a large one"""
    if n <= cap:
        return torch.arange(n)
    return (torch.arange(cap, dtype=torch.float64) * (n - 1) / (cap - 1)).round().long()


# ------------------------------------------------------------------------------------------------ head-module cases
HEAD_CASES = {
    "cosine_h256": dict(seed=11, B=24, kwargs=dict(head_name="gene", batch_key="gene_label", in_dims=768, hidden_dims=256,
                                                    num_classes=1001, cosine_classifier=True, top_k=5)),
    "linear_h64_32": dict(seed=12, B=10, kwargs=dict(head_name="marker", batch_key="marker_label", in_dims=48,
                                                      hidden_dims=[64, 32], num_classes=11, cosine_classifier=False, top_k=3)),
}
OPS_HEAD = dict(head_name="gene", batch_key="gene_label", in_dims=768, hidden_dims=256, num_classes=1001, cosine_classifier=True,
                loss_weight=0.5, top_k=5, weight_schedule="cosine", weight_start=0.0, weight_warmup_epochs=30)
SCHEDULE_EPOCHS = (0, 1, 15, 30, 31)


def build_head_case(name: str, cls=None) -> dict:
    """the head (``cls``: this module's restatement by default) under the case's seed, in training mode, with non-trivial
    BatchNorm affine parameters and running statistics, and its input"""
    c = HEAD_CASES[name]
    torch.manual_seed(c["seed"])
    head = (cls or ClassificationHead)(**c["kwargs"]).train()
    g = torch.Generator().manual_seed(c["seed"] + 1000)
    with torch.no_grad():
        for m in head.modules():
            if isinstance(m, nn.BatchNorm1d):
                m.weight.copy_(1 + 0.2 * torch.randn(m.weight.shape, generator=g))
                m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
                m.running_mean.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
                m.running_var.copy_(1 + 0.2 * torch.rand(m.bias.shape, generator=g))
    kw = c["kwargs"]
    x = torch.randn(c["B"], kw["in_dims"], generator=g)
    y = torch.randint(0, kw["num_classes"], (c["B"],), generator=g)
    return dict(head=head, x=x, y=y, k=kw["top_k"])


def head_reference(case: dict, dtype=torch.float64) -> dict:
    """one training forward + backward (gradient times GOUT) of a copy of the case's head in ``dtype``: loss, accuracies, the
    input gradient, every parameter gradient and the buffers after the forward"""
    import copy

    head = copy.deepcopy(case["head"]).to(dtype).train()
    x = case["x"].to(dtype).clone().requires_grad_(True)
    logits = head(x)
    loss = head.compute_loss(logits, case["y"])
    (loss * GOUT).backward()
    top1, topk = accuracies(logits.detach(), case["y"], case["k"])
    out = dict(loss=loss.detach(), top1=top1, topk=topk, dx=x.grad)
    out["grads"] = {n: p.grad for n, p in head.named_parameters()}
    out["buffers"] = {n: b.detach().clone() for n, b in head.named_buffers()}
    return out


# ------------------------------------------------------------------------------------------------ module-level composition
SMALL = dict(embedding_dim=32, projection_dim=16, depths=(1, 1, 1, 1), dims=(16, 32, 48, 64))   # tests/test_triplet_cpu.py
MODULE_HEAD = dict(head_name="gene", batch_key="gene_label", in_dims=64, hidden_dims=16, num_classes=7, cosine_classifier=True,
                   loss_weight=0.5, top_k=3)
MODULE_B, MODULE_LR, TEMPERATURE, MARGIN = 6, 1e-3, 0.5, 0.5


def module_batch() -> dict:
    g = torch.Generator().manual_seed(17)
    a = torch.randn(MODULE_B, 1, 5, 32, 32, generator=g)
    return {"anchor": a, "positive": a + 0.5 * torch.randn(a.shape, generator=g), "negative": a + 0.5 * torch.randn(a.shape, generator=g),
            "gene_label": torch.tensor([3, 0, 6, 3, 1, 5])}


def oracle_module_step(kind: str) -> dict:
    """one training step of the reference composition on the CPU: separate train-mode forwards of the oracle encoder per view,
    NT-Xent (``kind`` "ntxent") or torch's TripletMarginLoss ("triplet"), the restated head on the anchor's embedding,
    total = contrastive + weight * head loss, backward, one ``torch.optim.AdamW(all parameters, lr)`` step"""
    from oracle import contrastive_ref as C

    enc = C.randomize_encoder_(C.ContrastiveEncoder("convnextv2_tiny", in_channels=1, in_stack_depth=5, **SMALL), seed=3).train()
    torch.manual_seed(21)
    head = ClassificationHead(**MODULE_HEAD).train()
    start = {"enc": {k: v.clone() for k, v in enc.state_dict().items()}, "head": {k: v.clone() for k, v in head.state_dict().items()}}
    batch = module_batch()
    emb, pa = enc(batch["anchor"])
    _, pp = enc(batch["positive"])
    logged = {}
    if kind == "ntxent":
        idx = torch.arange(MODULE_B)
        contrastive = C.NTXentLoss(temperature=TEMPERATURE)(torch.cat((pa, pp)), torch.cat((idx, idx)))
    else:
        _, pn = enc(batch["negative"])
        contrastive = nn.TripletMarginLoss(margin=MARGIN)(pa, pp, pn)
        logged.update({"metrics/cosine_similarity/positive/train": F.cosine_similarity(pa, pp, dim=1).mean().detach(),
                       "metrics/euclidean_distance/positive/train": F.pairwise_distance(pa, pp).mean().detach(),
                       "metrics/cosine_similarity_negative/train": F.cosine_similarity(pa, pn, dim=1).mean().detach(),
                       "metrics/euclidean_distance_negative/train": F.pairwise_distance(pa, pn).mean().detach()})
    logits = head(emb)
    y = batch["gene_label"]
    head_loss = head.compute_loss(logits, y)
    total = contrastive + head.get_weight() * head_loss
    logged["loss/train"] = contrastive.detach()
    head.log_metrics({"loss": head_loss.detach(), "logits": logits.detach(), "y": y}, lambda k, v: logged.update({k: v}), "train")
    total.backward()
    zy = logits.detach().gather(1, y[:, None])
    gap = (logits.detach() - zy).abs().scatter(1, y[:, None], float("inf")).min()
    grads = {"enc": {k: p.grad.clone() for k, p in enc.named_parameters()}, "head": {k: p.grad.clone() for k, p in head.named_parameters()}}
    torch.optim.AdamW(list(enc.parameters()) + list(head.parameters()), lr=MODULE_LR).step()
    after = {k: v.detach().clone() for k, v in head.state_dict().items()}
    return dict(start=start, batch=batch, total=total.detach(), logged=logged, grads=grads, head_after=after, label_gap=float(gap))
