"""The k-NN probe of OnlineEvalCallback, event-timed: viscy_amd.online_eval.knn_accuracy (vsx_row_inv_norm + vsx_knn_topk +
vsx_knn_vote, no N x N buffer) against a plain-torch statement of the same result — row-chunked ``x @ x.T``, a fold mask, ``topk``
and a vote by counting (the yardstick, not the code under test) — at N = 16 384 and N = 51 200 rows of d = 768, k = 20, 5 folds,
12 classes.  Also the peak device memory of both and whether they agree.  SIZES=16384,51200 REP=3 CHUNK=4096 select."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from viscy_amd import online_eval as OE  # noqa: E402

REP = int(os.environ.get("REP", 3))
CHUNK = int(os.environ.get("CHUNK", 4096))  # yardstick rows per block: 4096 x 51 200 fp32 = 0.8 GiB, fits at both sizes
D, K, FOLDS, CLASSES = 768, 20, 5, 12


def yardstick(x, y, fold, k):
    """-> accuracy (mean of per-fold accuracies), as knn_accuracy"""
    xn = x * (1.0 / x.norm(dim=1, keepdim=True))
    hit = torch.empty(x.shape[0], dtype=torch.float64, device=x.device)
    for lo in range(0, x.shape[0], CHUNK):
        s = xn[lo:lo + CHUNK] @ xn.T
        s.masked_fill_(fold[lo:lo + CHUNK, None] == fold[None, :], float("-inf"))
        nb = y[s.topk(k, dim=1).indices]
        votes = torch.zeros(nb.shape[0], CLASSES, dtype=torch.int32, device=x.device).scatter_add_(1, nb, torch.ones_like(nb, dtype=torch.int32))
        hit[lo:lo + CHUNK] = (votes.argmax(1) == y[lo:lo + CHUNK]).double()   # argmax: the first (smallest) label on a tie
    return float(torch.stack([hit[fold == f].mean() for f in range(FOLDS)]).mean())


def timed(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    vals = []
    for it in range(REP + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        if it:
            vals.append(e0.elapsed_time(e1))
    return sorted(vals)[len(vals) // 2], (torch.cuda.max_memory_allocated() - base) / 2 ** 20, out


for n in (int(v) for v in os.environ.get("SIZES", "16384,51200").split(",")):
    g = torch.Generator(device="cuda").manual_seed(n)
    y = torch.randint(0, CLASSES, (n,), device="cuda", generator=g)
    centres = torch.randn(CLASSES, 16, device="cuda", generator=g)
    x = (centres[y] + 1.5 * torch.randn(n, 16, device="cuda", generator=g)) @ (torch.randn(16, D, device="cuda", generator=g) / 4.0)
    y_host = y.cpu().numpy()
    fold_host = OE.stratified_kfold_ids(y_host, FOLDS)
    fold = torch.from_numpy(fold_host).cuda()
    t_k, m_k, a_k = timed(lambda: OE.knn_accuracy(x, y_host, fold_host, K, range(FOLDS)))
    t_y, m_y, a_y = timed(lambda: yardstick(x, y, fold, K))
    print(f"N {n} d {D} k {K} folds {FOLDS}: knn_accuracy {t_k:.1f} ms, peak {m_k:.0f} MiB, accuracy {a_k:.6f} | "
          f"torch yardstick (chunk {CHUNK}) {t_y:.1f} ms, peak {m_y:.0f} MiB, accuracy {a_y:.6f} | "
          f"ratio {t_y / t_k:.2f}x, {2.0 * n * n * D / t_k / 1e9:.1f} TFLOP/s fp32 in the kernel path", flush=True)
    del x, y, fold
    torch.cuda.empty_cache()
