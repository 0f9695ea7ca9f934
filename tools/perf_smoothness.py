"""Temporal smoothness on the device, timed: the kernels of csrc/smoothness.hip (vsx_standardize, vsx_pair_dist over the adjacent
and the random pair list, vsx_kde_gauss at n x 1000) with HIP events, and viscy_amd.smoothness.compute_embeddings_smoothness end to
end on the wall clock (the embeddings are on the device, as `predict` leaves them; the pair lists, the copies of the distances
and the host statistics are included), for N x d synthetic tracked embeddings: tracks of 20 .. 100 rows, a random walk each.
Yardstick: the reference's route on the host (sklearn StandardScaler, one scipy cdist call per pair, two gaussian_kde objects on
1000 points, find_peaks) where scipy and sklearn are importable, at HOST_ROWS rows ONLY and labelled as that size: one run,
nothing is extrapolated.

Bandwidth figures are the bytes a pass must move over its time: standardize 2 N d 4 B; a pair pass 2 P d 4 B of rows.  The density
pass is reported as Gaussian terms per second (n x 1000 float64 exp).  SHAPES=100000x768,1000000x768 REP=20 WARM=3 HOST_ROWS=20000 select."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from viscy_amd import ops  # noqa: E402
from viscy_amd import smoothness as S  # noqa: E402
from viscy_amd.reduce import StandardScaler  # noqa: E402

REP = int(os.environ.get("REP", 20))
WARM = int(os.environ.get("WARM", 3))
SHAPES = [tuple(int(v) for v in s.split("x")) for s in os.environ.get("SHAPES", "100000x768,1000000x768").split(",")]
HOST_ROWS = int(os.environ.get("HOST_ROWS", 20000))


class Ms(float):
    """a median in ms that remembers the fastest and the slowest of its runs"""

    def spread(self):
        return f"[{self.lo:.3f} .. {self.hi:.3f}]"


def median(vals):
    vals = sorted(vals)
    m = Ms(vals[len(vals) // 2])
    m.lo, m.hi = vals[0], vals[-1]
    return m


def timed(fn, rep=REP):
    """median device time in ms of `rep` runs after WARM untimed ones (with the fastest and slowest run), and the last result"""
    torch.cuda.synchronize()
    vals = []
    for it in range(rep + WARM):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        if it >= WARM:
            vals.append(e0.elapsed_time(e1))
    return median(vals), out


def tracked(n, d, seed):
    """-> (x float32 (n, d) on the device, obs): one random walk per track of 20 .. 100 rows, drawn on the device in slabs"""
    rng = np.random.RandomState(seed)
    lengths = []
    while sum(lengths) < n:
        lengths.append(int(min(rng.randint(20, 101), n - sum(lengths))))
    lengths = np.array(lengths)
    track = np.repeat(np.arange(len(lengths)), lengths)
    starts = np.cumsum(lengths) - lengths
    t = np.arange(n) - np.repeat(starts, lengths)
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.empty(n, d, device="cuda")
    for r0 in range(0, n, 1 << 17):
        m = min(1 << 17, n - r0)
        x[r0:r0 + m] = torch.randn(m, d, device="cuda", generator=g) * 0.35
    # walk = cumulative sum within a track: cumsum over all rows minus the sum before the track's first row
    x = torch.cumsum(x, dim=0)
    base = torch.zeros(len(lengths), d, device="cuda")
    base[1:] = x[torch.from_numpy(starts[1:] - 1).cuda()]
    track_d = torch.from_numpy(track).cuda()
    x -= base[track_d]
    x += (torch.randn(len(lengths), d, device="cuda", generator=g) * 2.0)[track_d]
    del base
    obs = {"fov_name": np.array([f"A/{k % 4}/0" for k in range(len(lengths))], dtype=object)[track], "track_id": track // 4, "t": t}
    return x, obs


def host_reference(x, obs):
    """the reference's loop, restated on scipy / sklearn -> seconds per stage"""
    import pandas as pd
    from scipy.signal import find_peaks
    from scipy.spatial.distance import cdist
    from scipy.stats import gaussian_kde
    from sklearn.preprocessing import StandardScaler as SkScaler

    out = {}
    t0 = time.perf_counter()
    z = SkScaler().fit_transform(x)
    out["StandardScaler"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    adj = []
    for _, sub in pd.DataFrame(obs).reset_index(drop=True).groupby(["fov_name", "track_id"]):
        if len(sub) > 1:
            tf = z[sub.index.values]
            for i in range(len(tf) - 1):
                adj.append(cdist(tf[i:i + 1], tf[i + 1:i + 2], metric="cosine")[0, 0])
    adj = np.array(adj)
    out["adjacent cdist loop"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    ri, rj = S.random_pairs(len(z), len(adj))
    rnd = np.array([cdist(z[i:i + 1], z[j:j + 1], metric="cosine")[0, 0] for i, j in zip(ri, rj)])
    out["random cdist loop"] = time.perf_counter() - t0
    for name, v in (("adjacent", adj), ("random", rnd)):
        t0 = time.perf_counter()
        grid = np.linspace(v.min(), v.max(), 1000)
        k = gaussian_kde(v)(grid)
        find_peaks(k, height=k.max() * 0.1)
        out[f"gaussian_kde {name} (n = {len(v)})"] = time.perf_counter() - t0
    return out, adj, rnd


def main():
    import pandas  # noqa: F401 - the pair builder imports it on its first call: keep that out of the first timed figure

    S.adjacent_pairs(np.array(["a", "a"], dtype=object), np.array([0, 0]), [1])
    print(f"kernel lines: HIP events, median of {REP} runs after {WARM} untimed ones [fastest .. slowest]; end to end: wall clock, the same counts")
    for n, d in SHAPES:
        x, obs = tracked(n, d, n)
        sc = StandardScaler().fit(x)
        mean, scale = torch.from_numpy(sc.mean_).cuda(), torch.from_numpy(np.ascontiguousarray(sc.scale_)).cuda()
        t_std, z = timed(lambda: ops.standardize(x, mean, scale))
        t0 = time.perf_counter()
        pi, pj, _, _ = S.adjacent_pairs(obs["fov_name"], obs["track_id"], [1])
        t_build = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        ri, rj = S.random_pairs(n, len(pi))
        t_rand = (time.perf_counter() - t0) * 1e3
        P = len(pi)
        dv = lambda a: torch.from_numpy(a.astype(np.int32)).cuda()  # noqa: E731
        pid, pjd, rid, rjd = dv(pi), dv(pj), dv(ri), dv(rj)
        print(f"(N, d) = ({n}, {d}): {P} adjacent pairs; pair lists on the host {t_build:.1f} ms, random draw {t_rand:.1f} ms\n"
              f"  standardize {t_std:.3f} ms {t_std.spread()} = {2 * n * d * 4 / t_std / 1e9:.2f} TB/s", flush=True)
        for metric in ("cosine", "euclidean"):
            t_adj, da = timed(lambda: ops.pair_dist(z, pid, pjd, metric, 0.0))
            t_rnd, dr = timed(lambda: ops.pair_dist(z, rid, rjd, metric, 0.0))
            print(f"  pair_dist {metric:9s}: adjacent {t_adj:.3f} ms {t_adj.spread()} = {2 * P * d * 4 / t_adj / 1e9:.2f} TB/s of rows, random "
                  f"{t_rnd:.3f} ms {t_rnd.spread()} = {2 * P * d * 4 / t_rnd / 1e9:.2f} TB/s", flush=True)
            if metric == "cosine":
                keep = (da, dr)
        for name, v in zip(("adjacent", "random"), keep):
            host = v.cpu().numpy()
            a = 1.0 / (2.0 * S._kde_cov(host))
            grid = torch.from_numpy(np.linspace(host.min(), host.max(), 1000)).cuda()
            t_kde, _ = timed(lambda: ops.kde_gauss(v, grid, a))
            print(f"  kde_gauss {name:8s} n = {P} x 1000: {t_kde:.3f} ms {t_kde.spread()} = {P * 1000 / t_kde / 1e9:.3f} T terms/s "
                  f"({ops.kde_chunks(P, 1000)} chunks x 2 tiles)", flush=True)

        class Ad:
            X = x
        Ad.obs = obs
        walls = []
        for _ in range(REP + WARM):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            stats, _, _ = S.compute_embeddings_smoothness(Ad)
            walls.append((time.perf_counter() - t0) * 1e3)
        wall = median(walls[WARM:])
        print(f"  compute_embeddings_smoothness end to end: {wall:.1f} ms {wall.spread()}; "
              f"smoothness_score {stats['smoothness_score']:.4f}, dynamic_range {stats['dynamic_range']:.4f}", flush=True)
        del x, z
        torch.cuda.empty_cache()

    try:
        import scipy
        import sklearn
    except ImportError:
        print("scipy / sklearn are not importable on this host: no CPU yardstick")
        return
    n, d = HOST_ROWS, SHAPES[0][1]
    x, obs = tracked(n, d, n)

    class Ad:
        X = x
    Ad.obs = obs
    t0 = time.perf_counter()
    stats, dist, _ = S.compute_embeddings_smoothness(Ad)
    t_dev = time.perf_counter() - t0
    stages, adj, rnd = host_reference(x.cpu().numpy(), obs)
    print(f"host yardstick AT N = {n} ROWS ONLY, d = {d} (scipy {scipy.__version__}, sklearn {sklearn.__version__}, "
          f"{os.environ.get('OMP_NUM_THREADS', '?')} threads, one run):")
    for k, v in stages.items():
        print(f"  {k}: {v:.2f} s")
    print(f"  total {sum(stages.values()):.2f} s; this package at the same {n} rows, end to end: {t_dev * 1e3:.1f} ms\n"
          f"  max |distance - scipy's|: adjacent {np.abs(dist['adjacent_frame_distribution'] - adj).max():.2e}, "
          f"random {np.abs(dist['random_frame_distribution'] - rnd).max():.2e}")


if __name__ == "__main__":
    main()
