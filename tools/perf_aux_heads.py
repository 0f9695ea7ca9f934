"""The DynaCLR auxiliary ClassificationHead, event-timed: forward + backward of viscy_amd.heads.ClassificationHead
(``in 768 -> 256 -> 1001``, cosine classifier, k = 5: the head of OPS-1000genes-lite) through ``loss_and_stats`` against the
torch-eager composition on the same GPU and in the same process — ``Linear``, ``BatchNorm1d``, ``ReLU``, ``F.normalize``, ``mm``,
``cross_entropy``, ``argmax`` and ``topk`` under autograd (the yardstick, not the code under test) — at B = 64, 256, 512.
Median of REP = 3 runs after a warm-up.  SIZES=64,256,512 REP=3 select; OUT=<file> also writes the lines there."""
import os
import sys

import torch
import torch.nn.functional as F
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from viscy_amd.heads import ClassificationHead  # noqa: E402

REP = int(os.environ.get("REP", 3))
IN, HID, C, K = 768, 256, 1001, 5


class Eager(nn.Module):
    def __init__(self):
        super().__init__()
        self.backbone = nn.Sequential(nn.Linear(IN, HID), nn.BatchNorm1d(HID), nn.ReLU(inplace=True))
        self.weight = nn.Parameter(torch.randn(C, HID) * 0.01)
        self.log_scale = nn.Parameter(torch.tensor(20.0).log())

    def forward(self, x, y):
        h = self.backbone(x)
        logits = self.log_scale.exp() * (F.normalize(h, dim=1) @ F.normalize(self.weight, dim=1).t())
        loss = F.cross_entropy(logits, y)
        with torch.no_grad():
            top1 = (logits.argmax(dim=1) == y).float().mean()
            topk = (logits.topk(K, dim=1).indices == y.unsqueeze(1)).any(dim=1).float().mean()
        return loss, top1, topk


def timed(fn):
    torch.cuda.synchronize()
    vals = []
    for it in range(REP + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        if it:
            vals.append(e0.elapsed_time(e1))
    return sorted(vals)[len(vals) // 2], out


def main():
    lines = ["python tools/perf_aux_heads.py on one MI355X (event-timed forward + backward, median of %d after 1 warm-up run; host "
             "work of both sides included)" % REP]
    torch.manual_seed(0)
    head = ClassificationHead("gene", "gene_label", IN, HID, C, top_k=K).cuda().train()
    eager = Eager().cuda().train()
    for b in (int(v) for v in os.environ.get("SIZES", "64,256,512").split(",")):
        g = torch.Generator(device="cuda").manual_seed(b)
        x = torch.randn(b, IN, device="cuda", generator=g)
        y = torch.randint(0, C, (b,), device="cuda", generator=g)

        def ours():
            xi = x.clone().requires_grad_(True)
            loss, stats = head.loss_and_stats(xi, y)
            loss.backward()
            return loss.detach(), stats["top1"], stats["topk"]

        def theirs():
            xi = x.clone().requires_grad_(True)
            loss, top1, topk = eager(xi, y)
            loss.backward()
            return loss.detach(), top1, topk

        t_k, o_k = timed(ours)
        t_y, o_y = timed(theirs)
        lines.append(f"B {b} in {IN} -> {HID} -> {C} k {K}: loss_and_stats + backward {t_k * 1e3:.0f} us (loss {o_k[0].item():.4f}) | "
                     f"torch eager {t_y * 1e3:.0f} us (loss {o_y[0].item():.4f}) | ratio {t_y / t_k:.2f}x")
        print(lines[-1], flush=True)
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
