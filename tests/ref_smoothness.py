"""Fixtures and float64 restatements for the temporal-smoothness tests (tests/test_smoothness_cpu.py, tests/test_gpu_smoothness.py)
and for tools/gen_golden_smoothness.py.  Needs numpy alone: no GPU, no viscy_amd, no scipy.

The inputs of every case are rebuilt from seeds here; tests/golden/smoothness.pt holds only what the reference computed on them.

Restatements, bit for bit what csrc/smoothness.hip computes (include/vsx.h states the formulas):
  standardize(x, mean, scale)   fl32(double(fl32(double(x) - mean)) / scale)
  pair_dist(x, pi, pj, metric, eps)   lane l adds features 4 l .. 4 l + 3, 256 + 4 l .. in ascending order, the 64 lanes are added
                                by the xor butterfly 32 .. 1; Euclidean rounds the difference, the square and the add separately
  kde_sums(data, grid, a)       sum_i exp(-a (grid - data_i)^2) summed in np.longdouble: the yardstick of vsx_kde_gauss, not bit-equal"""
import numpy as np

U = 2.0 ** -53          # unit round-off of float64
GRID = 1000             # points of find_distribution_peak's grid
KDE_TILE, KDE_CHUNK = 512, 1024   # VSX_KDE_TILE, VSX_KDE_CHUNK of include/vsx.h (the GPU test checks them against the library)


# ------------------------------------------------------------------------------------------------ bounds the issue sets
def pair_bound(d: int) -> float:
    """two float64 sums of d exactly representable products, whatever their order: absolute for cosine, relative for Euclidean"""
    return 4.0 * (d + 8) * U


def kde_bound(n: int) -> float:
    """relative, per grid value: all terms are positive, so any order errs by at most (n - 1) u; 4096 u covers exp and an
    argument of magnitude up to 745"""
    return 2.0 * (n + 4096) * U


def pair_tolerance(z: np.ndarray, pi, pj, metric: str) -> np.ndarray:
    """E_p: what a last-bit difference of mean_ / scale_ (at most 2 ulp of a standardised fp32 element) can move a distance by"""
    if metric == "cosine":
        return np.full(len(pi), 2.0 ** -19)
    z64 = z.astype(np.float64)
    nrm = np.sqrt((z64 * z64).sum(1))
    return 2.0 ** -21 * (nrm[pi] + nrm[pj])


# ------------------------------------------------------------------------------------------------ restatements
def standardize(x: np.ndarray, mean: np.ndarray, scale: np.ndarray) -> np.ndarray:
    assert x.dtype == np.float32 and mean.dtype == np.float64 and scale.dtype == np.float64
    centred = (x.astype(np.float64) - mean[None, :]).astype(np.float32)
    return (centred.astype(np.float64) / scale[None, :]).astype(np.float32)


def _lane_sums(prod: np.ndarray) -> np.ndarray:
    """prod (P, d) float64 terms -> (P,) their sum in the kernel's order.  Features past d are padded with +0.0, which changes no
    sum: every lane starts from +0.0 and can never hold -0.0"""
    P, d = prod.shape
    t = np.concatenate([prod, np.zeros((P, -d % 256))], axis=1).reshape(P, -1, 64, 4)   # [pair, round, lane, k]
    lanes = np.zeros((P, 64))
    for r in range(t.shape[1]):
        for k in range(4):
            lanes = lanes + t[:, r, :, k]
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[:, idx ^ o]
    return lanes[:, 0]


def pair_dist(x: np.ndarray, pi, pj, metric: str, eps: float = 0.0, block: int = 4096) -> np.ndarray:
    assert x.dtype == np.float32
    pi, pj = np.asarray(pi), np.asarray(pj)
    out = np.empty(len(pi), dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        for s in range(0, len(pi), block):
            u, v = x[pi[s:s + block]].astype(np.float64), x[pj[s:s + block]].astype(np.float64)
            if metric == "cosine":
                uv, uu, vv = _lane_sums(u * v), _lane_sums(u * u), _lane_sums(v * v)
                den = np.maximum(np.sqrt(uu), eps) * np.maximum(np.sqrt(vv), eps)
                out[s:s + block] = 1.0 - uv / den
            elif metric == "euclidean":
                diff = u - v
                out[s:s + block] = np.sqrt(_lane_sums(diff * diff))
            else:
                raise ValueError(metric)
    return out


def kde_sums(data: np.ndarray, grid: np.ndarray, a: float, block: int = 4096) -> np.ndarray:
    """float64 terms exp(-a (g - x)^2), summed in long double"""
    acc = np.zeros(len(grid), dtype=np.longdouble)
    for s in range(0, len(data), block):
        dlt = grid[:, None] - data[None, s:s + block]
        acc += np.exp(-(a * (dlt * dlt))).astype(np.longdouble).sum(1)
    return acc


def kde_curve(data: np.ndarray, sums: np.ndarray) -> np.ndarray:
    """scipy's gaussian_kde values from the unnormalised sums: Scott's factor, cov = var(ddof=1) factor^2"""
    n = len(data)
    cov = float(np.var(data, ddof=1)) * float(n) ** -0.4
    return np.asarray(sums, dtype=np.float64) / (n * np.sqrt(2.0 * np.pi * cov))


def kde_a(data: np.ndarray) -> float:
    return 1.0 / (2.0 * float(np.var(data, ddof=1)) * float(len(data)) ** -0.4)


def random_pairs(n_samples: int, n_pairs: int):
    """the reference's baseline draw -> (i, j, redraws): RandomState(42), batches of 10 000, i then j, i == j redrawn"""
    rs = np.random.RandomState(42)
    I, J, redraws = [], [], 0
    for b0 in range(0, n_pairs, 10000):
        bn = min(b0 + 10000, n_pairs) - b0
        i = rs.randint(0, n_samples, size=bn)
        j = rs.randint(0, n_samples, size=bn)
        mask = i == j
        while mask.any():
            j[mask] = rs.randint(0, n_samples, size=mask.sum())
            mask = i == j
            redraws += 1
        I.append(i), J.append(j)
    return np.concatenate(I), np.concatenate(J), redraws


def adjacent_pairs_loop(fov, track, offsets):
    """the reference's loops, plainly -> (pi, pj, piecewise index lists): groups in sorted (fov_name, track_id) order, rows in row
    order, then offsets as given, then ascending i"""
    keys = sorted(set(zip(fov.tolist(), track.tolist())))
    pi, pj, pieces = [], [], []
    for key in keys:
        rows = [r for r in range(len(fov)) if (fov[r], track[r]) == key]
        if len(rows) > 1:
            mine = []
            for off in offsets:
                for i in range(len(rows) - off):
                    if off == 1:
                        mine.append(len(pi))
                    pi.append(rows[i]), pj.append(rows[i + off])
            if mine:
                pieces.append(mine)
    return np.array(pi, dtype=np.int64), np.array(pj, dtype=np.int64), pieces


HAND_MADE_PEAKS = [     # (signal, absolute height, the peaks scipy's rule gives)
    ([0, 1, 0], 0.0, [1]),
    ([0, 2, 2, 2, 0, 1, 0], 0.0, [2, 5]),                # a plateau gives its middle sample
    ([0, 2, 2, 2, 2, 0], 0.0, [2]),                       # (1 + 4) // 2
    ([3, 1, 0, 1, 3], 0.0, []),                           # the maxima sit on the edges
    ([0, 1, 0, 5, 0], 0.5 * 5, [3]),                      # a peak below the height
    ([0, 1, 1], 0.0, []),                                 # a plateau that runs into the edge
    ([0, 1, 2, 2, 3, 0], 0.0, [4]),                       # a shoulder is no peak
    ([1, 1, 1, 1], 0.0, []),
    ([0, 1, 0], 1.0, [1]),                                # height is inclusive
    ([5], 0.0, []),
]


def peak_signals():
    """what find_peaks(height=0.1 max) is recorded on: the hand-made signals and 20 random ones of many plateaus"""
    rng = np.random.RandomState(5)
    return [np.array(y, dtype=np.float64) for y, _, _ in HAND_MADE_PEAKS] + [rng.randint(0, 4, 60).astype(np.float64) for _ in range(20)]


# ------------------------------------------------------------------------------------------------ the cases
class Adata:
    """the duck type compute_embeddings_smoothness reads: .X and .obs"""

    def __init__(self, X, obs):
        self.X, self.obs = X, obs


def _walks(rng, lengths, d, step=0.35):
    """one random walk per track: neighbours in time are closer than random rows"""
    rows = []
    for L in lengths:
        start = rng.standard_normal(d) * 2.0
        rows.append(start[None, :] + np.cumsum(rng.standard_normal((L, d)) * step, axis=0))
    return np.concatenate(rows).astype(np.float32)


def _obs(lengths, fovs):
    fov = np.concatenate([np.full(L, fovs[k % len(fovs)], dtype=object) for k, L in enumerate(lengths)])
    track = np.concatenate([np.full(L, k // len(fovs), dtype=np.int64) for k, L in enumerate(lengths)])
    t = np.concatenate([np.arange(L, dtype=np.int64) for L in lengths])
    return {"fov_name": fov, "track_id": track, "t": t}


def _lengths_c(rng):
    out = []
    while sum(out) < 12000:
        out.append(int(min(rng.randint(6, 51), 12000 - sum(out))))
    if out[-1] < 6:   # keep every track within 6 .. 50 rows
        out[-2] -= 6 - out[-1]
        out[-1] = 6
    return out


CASES = {
    "A": dict(seed=11, d=16, lengths=[1, 2, 3, 7, 5, 9, 4, 6, 3], metric="cosine", offsets=[1]),
    "B": dict(seed=12, d=16, lengths=[1, 2, 3, 7, 4, 6, 10, 5, 2], metric="euclidean", offsets=[1, 2, 5]),
    "C": dict(seed=13, d=8, lengths="c", metric="cosine", offsets=[1]),
    "D": dict(seed=14, d=4, lengths=[3], metric="cosine", offsets=[1, 2]),
    "E": dict(seed=15, d=6, lengths=[6, 1, 8, 5, 7, 3], metric="cosine", offsets=[1, 2], shuffle=True),
    "F": dict(seed=16, d=5, lengths=[1, 1, 1, 1, 1], metric="cosine", offsets=[1]),
    "G": dict(seed=17, d=768, lengths=[30, 10, 25, 1, 17, 22, 28, 12, 19, 30, 26, 14, 21, 11, 20, 14], metric="cosine", offsets=[1]),
    "H": dict(seed=18, d=5, lengths=[4, 9, 1, 12, 6, 8], metric="euclidean", offsets=[1], constant_column=2),
}
FOVS = ("B/2/0", "A/1/0", "A/1/1")


def build(name: str):
    """-> (x float32 (N, d), obs dict of arrays, metric, offsets)"""
    c = CASES[name]
    rng = np.random.RandomState(c["seed"])
    lengths = _lengths_c(rng) if c["lengths"] == "c" else c["lengths"]
    x = _walks(rng, lengths, c["d"])
    obs = _obs(lengths, FOVS)
    if "constant_column" in c:
        x[:, c["constant_column"]] = 3.25
    if c.get("shuffle"):   # rows of several tracks interleaved and not in t order
        perm = rng.permutation(len(x))
        x, obs = np.ascontiguousarray(x[perm]), {k: v[perm] for k, v in obs.items()}
    return x, obs, c["metric"], list(c["offsets"])


def adata(name: str, frame: bool = False):
    x, obs, metric, offsets = build(name)
    if frame:
        import pandas as pd

        obs = pd.DataFrame(obs, index=[f"cell{i}" for i in range(len(x))])
    return Adata(x, obs), metric, offsets


def msd_dataset():
    """two FOVs reusing track_id 3, non-unit t steps, a 1-row track, rows interleaved and out of t order, one all-zero row;
    every track has at most 25 rows (torch.cdist switches to the matmul form past that, with a cancellation error no pair bound covers)"""
    rng = np.random.RandomState(21)
    lengths, fovs, tracks = [5, 1, 7, 4, 12], ["A/1/0", "A/1/0", "B/2/0", "B/2/0", "A/1/1"], [3, 4, 3, 9, 0]
    x = _walks(rng, lengths, 12)
    fov = np.concatenate([np.full(L, f, dtype=object) for L, f in zip(lengths, fovs)])
    track = np.concatenate([np.full(L, k, dtype=np.int64) for L, k in zip(lengths, tracks)])
    t = np.concatenate([np.sort(rng.choice(40, L, replace=False)).astype(np.int64) for L in lengths])
    x[8] = 0.0
    perm = rng.permutation(len(x))
    return {"features": np.ascontiguousarray(x[perm]), "fov_name": fov[perm], "track_id": track[perm], "t": t[perm]}


DEGENERATE = {"one_value": np.array([0.5]), "zero_variance": np.array([2.0, 2.0, 2.0]), "empty": np.array([])}
