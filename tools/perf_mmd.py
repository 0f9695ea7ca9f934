"""The MMD permutation test, event-timed: viscy_amd.mmd.mmd_permutation_test (vsx_mmd_prepare + vsx_mmd_sums, no N x N buffer; the
host's label draws and copies included) against two yardsticks that do what the reference does — materialise the pooled N x N
float32 kernel and multiply it by the (N, P) label matrix twice:
  torch   on the same device (torch.cdist, exp, two matmuls), labels drawn by the same host code;
  numpy   the reference's expressions without float64 (Gram-form distances instead of scipy's float64 cdist) on the host's
          threads, at the first shape only, one run.
Shapes (n, m, d, P): the recipe's max_cells 2000 + 2000 and the reference's cap 10 000 + 10 000, d = 768, P = 1000.  Reported:
median time after a warm-up, peak device memory, the fp32 TFLOP/s of both products (2 N^2 d + 2 N^2 P flop) in the kernel-only
time, and the largest difference between the two devices' results.  SHAPES=2000x2000x768x1000,... REP=3 NUMPY=1 select."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from viscy_amd import mmd as M  # noqa: E402
from viscy_amd import ops  # noqa: E402

REP = int(os.environ.get("REP", 3))
SHAPES = [tuple(int(v) for v in s.split("x")) for s in os.environ.get("SHAPES", "2000x2000x768x1000,10000x10000x768x1000").split(",")]
SEED = 42


def mmd2_from_sums(sxx, syy, sxy, n, m):
    return sxx / (n * (n - 1.0)) + syy / (m * (m - 1.0)) - 2.0 * sxy / (float(n) * m)


def torch_yardstick(X, Y, P, bw):
    """the reference's mmd_permutation_test in torch on the device: (N, N) float32 kernel, K @ z.T and K @ (1 - z).T"""
    n, m = len(X), len(Y)
    pool = torch.cat((X, Y))
    K = torch.exp(torch.cdist(pool, pool).square_() / (-2.0 * bw))
    K.fill_diagonal_(0.0)
    z = torch.from_numpy(M.permutation_labels(n, m, P, SEED)).to(X.device).float()
    KzT, KcT = K @ z.T, K @ (1 - z).T
    sxx, syy, sxy = (z * KzT.T).sum(1), ((1 - z) * KcT.T).sum(1), (z * KcT.T).sum(1)
    v = mmd2_from_sums(sxx.double(), syy.double(), sxy.double(), n, m).cpu().numpy()
    return float(v[0]), float((np.sum(v[1:] >= v[0]) + 1) / (P + 1)), v[1:]


def numpy_yardstick(X, Y, P, bw):
    n, m = len(X), len(Y)
    pool = np.concatenate([X, Y]).astype(np.float32)
    nrm = (pool * pool).sum(1)
    sq = np.maximum(nrm[:, None] + nrm[None, :] - np.float32(2) * (pool @ pool.T), np.float32(0))
    K = np.exp(sq / np.float32(-2.0 * bw), dtype=np.float32)
    np.fill_diagonal(K, 0.0)
    z = M.permutation_labels(n, m, P, SEED).astype(np.float32)
    KzT, KcT = K @ z.T, K @ (1 - z).T
    v = mmd2_from_sums((z * KzT.T).sum(1), ((1 - z) * KcT.T).sum(1), (z * KcT.T).sum(1), n, m)
    return float(v[0]), float((np.sum(v[1:] >= v[0]) + 1) / (P + 1)), v[1:]


def timed(fn, rep=REP):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    vals = []
    for it in range(rep + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        if it:
            vals.append(e0.elapsed_time(e1))
    return sorted(vals)[len(vals) // 2], (torch.cuda.max_memory_allocated() - base) / 2 ** 20, out


for si, (n, m, d, P) in enumerate(SHAPES):
    N = n + m
    g = torch.Generator(device="cuda").manual_seed(N)
    X = torch.randn(n, d, device="cuda", generator=g) + 0.5
    Y = torch.randn(m, d, device="cuda", generator=g) + 0.5 + 0.02
    t_bw, _, bw = timed(lambda: M.median_heuristic(X, Y))
    t0 = time.perf_counter()
    labels = M.permutation_labels(n, m, P, SEED)
    t_draw = (time.perf_counter() - t0) * 1e3
    t_all, mem_all, (obs, p, null) = timed(lambda: M.mmd_permutation_test(X, Y, n_permutations=P, bandwidth=bw, seed=SEED))
    pool = torch.cat((X, Y))
    z = torch.from_numpy(labels).cuda()
    t_prep, _, (xc, norms, _) = timed(lambda: ops.mmd_prepare(pool))
    t_sums, _, _ = timed(lambda: ops.mmd_sums(xc, norms, z, bw))
    t_one, _, _ = timed(lambda: ops.mmd_sums(xc, norms, z[:1].contiguous(), bw))
    flop = 2.0 * N * N * (d + P + 1)
    t_y, mem_y, (obs_y, p_y, null_y) = timed(lambda: torch_yardstick(X, Y, P, bw))
    diff = max(abs(obs - obs_y), float(np.abs(null - null_y).max()))
    print(f"(n, m, d, P) = ({n}, {m}, {d}, {P}), bandwidth {bw:.3f} (median_heuristic {t_bw:.1f} ms):\n"
          f"  mmd_permutation_test {t_all:.1f} ms, peak {mem_all:.0f} MiB  [host label draw {t_draw:.1f} ms of it; on the device: prepare "
          f"{t_prep:.2f} ms, sums {t_sums:.2f} ms = {flop / t_sums / 1e9:.1f} TFLOP/s fp32 over both products; sums with P = 1 "
          f"{t_one:.2f} ms = {2.0 * N * N * (d + 2) / t_one / 1e9:.1f} TFLOP/s]\n"
          f"  torch yardstick {t_y:.1f} ms, peak {mem_y:.0f} MiB  | ratio {t_y / t_all:.2f}x  | mmd2 {obs:.6e} / {obs_y:.6e}, p {p:.4f} / {p_y:.4f}, "
          f"max |difference| over mmd2 and the null {diff:.2e}", flush=True)
    if si == 0 and int(os.environ.get("NUMPY", 1)):
        Xh, Yh = X.cpu().numpy(), Y.cpu().numpy()
        t0 = time.perf_counter()
        obs_n, p_n, null_n = numpy_yardstick(Xh, Yh, P, bw)
        t_n = (time.perf_counter() - t0) * 1e3
        print(f"  numpy yardstick ({os.environ.get('OMP_NUM_THREADS', '?')} threads, one run) {t_n:.0f} ms  | mmd2 {obs_n:.6e}, p {p_n:.4f}, "
              f"max |difference| {max(abs(obs - obs_n), float(np.abs(null - null_n).max())):.2e}", flush=True)
    del X, Y, pool, xc, norms, z
    torch.cuda.empty_cache()
