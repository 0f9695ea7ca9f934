"""Clustering evaluation on the device, timed: the kernels of csrc/clustering.hip with HIP events and
viscy_amd.clustering.dbscan_clustering end to end on the wall clock (the embeddings are on the device; the round loop's host
reads and the copy of the labels are included), for N x d synthetic embeddings: CLUSTERS Gaussian blobs whose rows lie about
0.43 apart, and one row in a hundred far from everything.  Medians of REP runs after WARM untimed ones.

  vsx_pdist_f64    a block of BLOCK rows x N columns, Euclidean: TFLOP/s on 2 rows N d.  No share of a peak is printed: the
                   hardware notes this repository works from state no float64 matrix peak
  vsx_eps_graph    the whole bit matrix at eps = 0.5: TFLOP/s on 2 N^2 d
  the rounds       vsx_cc_round until nothing changes: their count and total time
  dbscan_clustering end to end
Yardsticks on the same box: torch's own float64 path for the same block (x.double() @ x.double().T and the same epilogue), and
sklearn's DBSCAN on the host at HOST_ROWS rows ONLY, one run, where sklearn is importable (said so where it is not).

SHAPES=20000x768,100000x768 REP=20 WARM=3 BLOCK=8192 CLUSTERS=50 HOST_ROWS=20000 select."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from viscy_amd import clustering as CL  # noqa: E402
from viscy_amd import ops  # noqa: E402

REP = int(os.environ.get("REP", 20))
WARM = int(os.environ.get("WARM", 3))
BLOCK = int(os.environ.get("BLOCK", 8192))
CLUSTERS = int(os.environ.get("CLUSTERS", 50))
SHAPES = [tuple(int(v) for v in s.split("x")) for s in os.environ.get("SHAPES", "20000x768,100000x768").split(",")]
HOST_ROWS = int(os.environ.get("HOST_ROWS", 20000))
EPS, MIN_SAMPLES = 0.5, 5


class Ms(float):
    """a median in ms that remembers the fastest and the slowest of its runs"""

    def spread(self):
        return f"[{self.lo:.3f} .. {self.hi:.3f}]"


def median(vals):
    vals = sorted(vals)
    m = Ms(vals[len(vals) // 2])
    m.lo, m.hi = vals[0], vals[-1]
    return m


def timed(fn, wall=False):
    """median time in ms of REP runs after WARM untimed ones (device events, or the wall clock around a synchronised run)"""
    torch.cuda.synchronize()
    vals = []
    for it in range(REP + WARM):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        if it >= WARM:
            vals.append((time.perf_counter() - t0) * 1e3 if wall else e0.elapsed_time(e1))
    return median(vals), out


def blobs(n, d, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    centres = torch.randn(CLUSTERS, d, device="cuda", generator=g) * (2.0 / d ** 0.5)       # about 2.8 apart
    member = torch.randint(0, CLUSTERS, (n,), device="cuda", generator=g)
    x = torch.empty(n, d, device="cuda")
    for r0 in range(0, n, 1 << 16):
        r1 = min(r0 + (1 << 16), n)
        x[r0:r1] = centres[member[r0:r1]] + torch.randn(r1 - r0, d, device="cuda", generator=g) * (0.43 / (2.0 * d) ** 0.5)
    far = torch.arange(0, n, 100, device="cuda")
    x[far] += torch.randn(len(far), d, device="cuda", generator=g) * (3.0 / d ** 0.5)
    return x


def torch_block(x64, n64, r0, r1):
    """the float64 yardstick: the same Euclidean block from torch's own matmul"""
    g = x64[r0:r1] @ x64.T
    out = (n64[r0:r1, None] + n64[None, :] - 2.0 * g).clamp_min_(0.0).sqrt_()
    out[torch.arange(r1 - r0, device=x64.device), torch.arange(r0, r1, device=x64.device)] = 0.0
    return out


def rounds(adj, core, labels, changed, index):
    labels.copy_(index)
    for count in range(1, len(index) + 2):
        ops.cc_round(adj, core, labels, changed)
        if int(changed.item()) == 0:
            return count
    raise RuntimeError("the components did not settle")


def main():
    print(f"device {torch.cuda.get_device_name(0)}; REP {REP} WARM {WARM}; eps {EPS} min_samples {MIN_SAMPLES}; {CLUSTERS} blobs", flush=True)
    for n, d in SHAPES:
        x = blobs(n, d, 7)
        rows = min(BLOCK, n)
        print(f"\n{n} x {d}:", flush=True)
        t_norm, norms = timed(lambda: ops.row_sqnorm_f64(x))
        print(f"  vsx_row_sqnorm_f64: {t_norm:.3f} ms {t_norm.spread()}")
        out = torch.empty((rows, n), dtype=torch.float64, device="cuda")
        t_pd, _ = timed(lambda: ops.pdist_f64(x, norms, "euclidean", rows=(0, rows), out=out))
        flops = 2.0 * rows * n * d
        print(f"  vsx_pdist_f64 {rows} x {n} euclidean: {t_pd:.3f} ms {t_pd.spread()} = {flops / t_pd / 1e9:.2f} TFLOP/s, "
              f"{rows * n * 8 / t_pd / 1e9:.2f} TB/s of output")
        x64 = x.double()
        n64 = (x64 * x64).sum(dim=1)
        t_th, ref = timed(lambda: torch_block(x64, n64, 0, rows))
        t_mm, _ = timed(lambda: x64[:rows] @ x64.T)
        print(f"  torch float64, the same block: {t_th:.3f} ms {t_th.spread()} = {flops / t_th / 1e9:.2f} TFLOP/s (its matmul alone {t_mm:.3f} ms = "
              f"{flops / t_mm / 1e9:.2f} TFLOP/s); vsx / torch = {t_pd / t_th:.2f}")
        print(f"  max |vsx - torch| on the block: {float((out - ref).abs().max()):.3e}", flush=True)
        del out, ref, x64, n64
        words = ops.eps_graph_words(n)
        adj = torch.empty((n, words), dtype=torch.int64, device="cuda")
        deg = torch.empty(n, dtype=torch.int32, device="cuda")
        t_g, _ = timed(lambda: ops.eps_graph(x, norms, EPS * EPS, adj, deg))
        print(f"  vsx_eps_graph ({n * words * 8 / 2 ** 20:.0f} MiB of bits): {t_g:.3f} ms {t_g.spread()} = {2.0 * n * n * d / t_g / 1e9:.2f} TFLOP/s; "
              f"mean degree {float(deg.double().mean()):.1f}")
        core = (deg >= MIN_SAMPLES).to(torch.uint8)
        index = torch.arange(n, dtype=torch.int32, device="cuda")
        labels, changed = torch.empty_like(index), torch.empty(1, dtype=torch.int32, device="cuda")
        t_r, count = timed(lambda: rounds(adj, core, labels, changed, index), wall=True)
        print(f"  the rounds: {count} of vsx_cc_round, {t_r:.3f} ms {t_r.spread()} on the wall clock (one host read per round)")
        del adj, deg
        t_e, lab = timed(lambda: CL.dbscan_clustering(x, EPS, MIN_SAMPLES), wall=True)
        print(f"  dbscan_clustering end to end: {t_e:.1f} ms {t_e.spread()}; {lab.max() + 1} clusters, {(lab < 0).sum()} noise rows", flush=True)
        if n == HOST_ROWS:
            try:
                from sklearn.cluster import DBSCAN
            except ImportError:
                print(f"  sklearn is not importable here: no host yardstick at {n} rows")
                continue
            host = x.cpu().numpy()
            t0 = time.perf_counter()
            sk = DBSCAN(eps=EPS, min_samples=MIN_SAMPLES).fit_predict(host)
            dt = time.perf_counter() - t0
            print(f"  sklearn DBSCAN on the host, {n} rows ONLY, one run: {dt:.1f} s ({os.cpu_count()} CPUs visible); labels equal: {np.array_equal(sk, lab)}"
                  f"; rows that differ: {int((sk != lab).sum())}", flush=True)


if __name__ == "__main__":
    main()
