"""Temporal smoothness of embeddings on the device: ``compute_embeddings_smoothness`` and ``find_distribution_peak`` of
``viscy_utils.evaluation.smoothness`` (what ``dynaclr evaluate-smoothness`` calls once per model and ``group_by`` value) and
``compute_track_displacement`` of ``viscy_utils.evaluation.distance``, with the reference's names, keywords, defaults, return types
and exceptions.

The reference calls ``cdist`` on two one-row slices about 2 N times and evaluates two ``gaussian_kde`` objects point by point.  Here
the host builds the pair lists (vectorised, in the reference's order) and the device does the arithmetic (csrc/smoothness.hip):

    vsx_standardize   sklearn's StandardScaler.transform of a float32 matrix, bit for bit, from this package's mean_ / scale_
    vsx_pair_dist     float64 cosine / Euclidean distances of listed row pairs, one wave per pair, one summation order
    vsx_kde_gauss     sum_i exp(-a (grid_g - data_i)^2) on the 1000-point grid, float64, fixed-order sums

What stays on the host is O(pairs): mean / std / median, the normalisation of the density and scipy's ``find_peaks(height=)`` restated
in numpy.  The distances come back as float64 arrays because the return type asks for them.  There is no CPU path for the three
passes: without a HIP device the functions raise ``RuntimeError``.  scipy and sklearn are not imported.  Input handling is
``evalkit``'s; the features are not checked for finite values here (``StandardScaler.fit`` does that for the smoothness).

Deliberate differences from the reference:

* ``mean_`` / ``scale_`` are this package's (float64 two-pass moments); they may differ from sklearn's in the last bit, which moves
  a standardised element by at most 2 float32 ulp;
* ``compute_track_displacement`` serves "cosine" and "euclidean" and raises ``ValueError`` for any other metric (the reference
  falls back to scipy there);
* a time offset below 1 raises ``ValueError``.
"""

from __future__ import annotations

from collections.abc import Mapping

import numpy as np
import torch

from .evalkit import as_matrix, column, device_of, to_device, upload

__all__ = ["find_distribution_peak", "compute_embeddings_smoothness", "compute_track_displacement", "adjacent_pairs", "random_pairs",
           "track_pairs", "find_peaks_height", "kde_curve"]

GRID_POINTS = 1000
HIST_BINS = 50
RANDOM_BATCH = 10000
MSD_CHUNK = 1 << 22     # pairs per vsx_pair_dist call of compute_track_displacement: 2 x 16 MiB of indices, 32 MiB of distances


# ------------------------------------------------------------------------------------------------ host: pure functions
def find_peaks_height(y: np.ndarray, height: float) -> np.ndarray:
    """scipy.signal.find_peaks(y, height=height) -> the peak indices: strict local maxima, a plateau higher than both its
    neighbours contributes its middle sample ``(left + right) // 2``, the two ends are never peaks; then ``y[peak] >= height``"""
    y = np.asarray(y, dtype=np.float64)
    if y.size < 3:
        return np.zeros(0, dtype=np.intp)
    change = np.flatnonzero(y[1:] != y[:-1])           # a run of equal samples ends at change[k], the next begins at change[k] + 1
    starts = np.concatenate(([0], change + 1))
    ends = np.concatenate((change, [y.size - 1]))
    inner = np.arange(1, len(starts) - 1)               # runs that have a neighbour on both sides
    v = y[starts]
    is_peak = (v[inner] > v[inner - 1]) & (v[inner] > v[inner + 1])
    peaks = (starts[inner][is_peak] + ends[inner][is_peak]) // 2
    return peaks[y[peaks] >= height].astype(np.intp)


def _highest_peak(x: np.ndarray, y: np.ndarray):
    peaks = find_peaks_height(y, np.max(y) * 0.1)
    if len(peaks) == 0:
        return x[np.argmax(y)]
    return x[peaks[np.argmax(y[peaks])]]


def kde_curve(data, sums) -> np.ndarray:
    """scipy's ``gaussian_kde(data)(grid)`` from the device's unnormalised sums: ``sums / (n sqrt(2 pi cov))``"""
    n = len(data)
    return np.asarray(sums, dtype=np.float64) / (n * np.sqrt(2.0 * np.pi * _kde_cov(data)))


def _kde_cov(data: np.ndarray) -> float:
    """Scott's rule for one dimension: var(ddof=1) n^(-2/5); the reference's exceptions for a degenerate sample"""
    data = np.atleast_1d(np.asarray(data, dtype=np.float64))
    if data.ndim != 1:
        raise ValueError("data must be one-dimensional")
    if data.size < 2:
        raise ValueError("`dataset` input should have multiple elements.")
    cov = float(np.var(data, ddof=1)) * float(data.size) ** -0.4
    if not cov > 0.0:
        raise np.linalg.LinAlgError(
            "The data appears to lie in a lower-dimensional subspace of the space in which it is expressed. This has resulted in a "
            "singular data covariance matrix, which cannot be treated using the algorithms implemented in `gaussian_kde`. Consider "
            "performing principal component analysis / dimensionality reduction and using `gaussian_kde` with the transformed data.")
    return cov


def _codes(values) -> tuple[np.ndarray, int]:
    """-> (the rank of every value among the sorted distinct values, how many there are)"""
    arr = column(values)
    if arr.dtype == object:   # names: hashed once and only the distinct ones sorted, as groupby does; 6 x np.unique at 10^6 rows
        import pandas as pd

        codes, uniq = pd.factorize(arr, sort=True)
        if (codes < 0).any():
            raise ValueError("fov_name and track_id must not hold missing values")
        return codes.astype(np.int64), len(uniq)
    uniq, inv = np.unique(arr, return_inverse=True)
    return inv.reshape(-1).astype(np.int64), len(uniq)


def _track_keys(fov, track) -> np.ndarray:
    """one int64 per row that orders the rows as ``groupby(["fov_name", "track_id"])`` orders its groups"""
    f, _ = _codes(fov)
    t, nt = _codes(track)
    if len(f) != len(t):
        raise ValueError("fov_name and track_id must have one entry per row")
    return f * nt + t


def adjacent_pairs(fov, track, time_offsets) -> tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """The reference's loops as arrays -> (pi, pj, piecewise, piecewise_splits): groups in sorted (fov_name, track_id) order, the
    rows of a group in ROW order (not sorted by t), then the offsets in the given order, then ascending i.  ``piecewise`` are the
    positions in the pair list that an offset of 1 produced and ``np.split(piecewise, piecewise_splits)`` the per-track lists"""
    offsets = np.asarray(list(time_offsets), dtype=np.int64).reshape(-1)
    if (offsets < 1).any():
        raise ValueError(f"time_offsets must be positive, got {list(time_offsets)}")
    key = _track_keys(fov, track)
    order = np.argsort(key, kind="stable")
    sorted_key = key[order]
    starts = np.flatnonzero(np.concatenate(([True], sorted_key[1:] != sorted_key[:-1]))) if len(key) else np.zeros(0, dtype=np.int64)
    lengths = np.diff(np.concatenate((starts, [len(key)])))
    counts = np.maximum(lengths[:, None] - offsets[None, :], 0)        # [group, offset]: a group of one row gives none
    flat = counts.reshape(-1)
    total = int(flat.sum())
    seg = np.repeat(np.arange(flat.size), flat)                         # the (group, offset) segment of every pair
    within = np.arange(total) - np.repeat(np.cumsum(flat) - flat, flat)
    g, o = seg // max(len(offsets), 1), seg % max(len(offsets), 1)
    pos_i = starts[g] + within
    pi, pj = order[pos_i], order[pos_i + offsets[o]]
    piecewise = np.flatnonzero(offsets[o] == 1)
    pg = g[piecewise]
    splits = np.flatnonzero(pg[1:] != pg[:-1]) + 1
    return pi.astype(np.int64), pj.astype(np.int64), piecewise, splits


def random_pairs(n_samples: int, n_pairs: int) -> tuple[np.ndarray, np.ndarray]:
    """the reference's baseline draw from a private ``RandomState(42)`` (the reference seeds the global one): batches of 10 000,
    ``randint(0, n, size)`` for i, then for j, and one ``randint`` of the masked size per pass while any i == j"""
    rs = np.random.RandomState(42)
    I, J = [], []
    for b0 in range(0, n_pairs, RANDOM_BATCH):
        bn = min(b0 + RANDOM_BATCH, n_pairs) - b0
        i = rs.randint(0, n_samples, size=bn)
        j = rs.randint(0, n_samples, size=bn)
        mask = i == j
        while mask.any():
            j[mask] = rs.randint(0, n_samples, size=mask.sum())
            mask = i == j
        I.append(i), J.append(j)
    return np.concatenate(I), np.concatenate(J)


def track_pairs(fov, track, t):
    """The pair order of ``compute_track_displacement`` -> (rows, starts, lengths): ``rows`` lists the row indices track by track, the
    tracks in first-appearance order, the rows of a track sorted by t (stably); track k is rows[starts[k] : starts[k] + lengths[k]].
    Its pairs are, for off = 1 .. T - 1 and ascending i, (i, i + off)"""
    key = _track_keys(fov, track)
    t = column(t)
    if len(t) != len(key):
        raise ValueError("t must have one entry per row")
    uniq, first, inv = np.unique(key, return_index=True, return_inverse=True)
    rank = np.empty(len(uniq), dtype=np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(uniq))
    appear = rank[inv.reshape(-1)]
    rows = np.lexsort((t, appear))                      # by track, then by t; lexsort is stable
    lengths = np.bincount(appear, minlength=len(uniq)).astype(np.int64)
    starts = np.cumsum(lengths) - lengths
    return rows.astype(np.int64), starts, lengths


def _offset_major(T: int, cache: dict) -> tuple[np.ndarray, np.ndarray]:
    """(i, j) of one track of T rows: off = 1 .. T - 1, ascending i"""
    if T not in cache:
        counts = np.arange(T - 1, 0, -1)              # T - off pairs at offset off
        off = np.repeat(np.arange(1, T), counts)
        i = np.arange(len(off)) - np.repeat(np.cumsum(counts) - counts, counts)
        cache[T] = (i.astype(np.int64), (i + off).astype(np.int64))
    return cache[T]


# ------------------------------------------------------------------------------------------------ input plumbing
def _features(X) -> torch.Tensor:
    """float32 (N, d) on the device; a device tensor is used in place.  The device is looked for first; the values are not"""
    dev = device_of(X, who="smoothness")
    return to_device(as_matrix(X, "features", finite=False, unwrap=True), dev)


def _pair_dist(x: torch.Tensor, pi: np.ndarray, pj: np.ndarray, metric: str, eps: float) -> np.ndarray:
    from . import ops

    if len(pi) and not (0 <= min(pi.min(), pj.min()) and max(pi.max(), pj.max()) < min(x.shape[0], 2 ** 31)):
        raise ValueError(f"pair indices must lie in [0, {min(x.shape[0], 2 ** 31)}): the kernel takes them as int32")
    return ops.pair_dist(x, upload(pi, x.device, np.int32), upload(pj, x.device, np.int32), metric, eps).cpu().numpy()


def _metric(distance_metric: str) -> str:
    if distance_metric not in ("cosine", "euclidean"):
        raise ValueError(f"distance_metric {distance_metric!r} is not served on the device: use 'cosine' or 'euclidean'")
    return distance_metric


# ------------------------------------------------------------------------------------------------ the reference's functions
def find_distribution_peak(data, method="kde_robust") -> float:
    """The peak of a distribution (the highest one if there are several).  ``"kde_robust"``: a Gaussian kernel density with Scott's
    bandwidth on ``linspace(min, max, 1000)`` (``vsx_kde_gauss``), peaks at least a tenth of the maximum high, the grid argmax where
    there is none; ``"histogram"``: the same rule on 50 density bins, on the host"""
    if method == "histogram":
        density, edges = np.histogram(column(data), bins=HIST_BINS, density=True)
        return _highest_peak(0.5 * (edges[:-1] + edges[1:]), density)
    elif method == "kde_robust":
        from . import ops

        host = np.ascontiguousarray(np.atleast_1d(np.asarray(column(data), dtype=np.float64)).reshape(-1))
        cov = _kde_cov(host)
        dev = device_of(data, who="smoothness")
        x_range = np.linspace(np.min(host), np.max(host), GRID_POINTS)
        sums = ops.kde_gauss(upload(host, dev), upload(x_range, dev), 1.0 / (2.0 * cov))
        return _highest_peak(x_range, kde_curve(host, sums.cpu().numpy()))
    else:
        raise ValueError(f"Unknown method: {method}. Use 'histogram' or 'kde_robust'.")


def compute_embeddings_smoothness(features_ad, distance_metric="cosine", time_offsets=[1], verbose=False):
    """-> (stats, distributions, piecewise_distance_per_track) as the reference.  ``features_ad`` is duck-typed: ``.X`` a numpy
    array or a tensor (one on the device is used in place), ``.obs`` a DataFrame or a mapping with ``fov_name``, ``track_id``, ``t``.
    The embeddings are standardised (``StandardScaler``), the distances of temporal neighbours within a track (all ``time_offsets``
    pooled) are compared with as many random pairs; ``piecewise_distance_per_track`` holds the offset-1 distances track by track"""
    from . import ops
    from .reduce import StandardScaler

    metric = _metric(distance_metric)
    say = print if verbose else (lambda *a: None)
    x = _features(features_ad.X)
    obs = features_ad.obs
    n_rows = len(column(obs["fov_name"]))
    if n_rows != x.shape[0]:
        raise ValueError(f"obs has {n_rows} rows, X {x.shape[0]}")
    scaler = StandardScaler().fit(x)
    z = ops.standardize(x, upload(scaler.mean_, x.device), upload(scaler.scale_, x.device))

    pi, pj, piecewise, splits = adjacent_pairs(obs["fov_name"], obs["track_id"], time_offsets)
    say(f"{len(pi)} pairs of temporal neighbours at offsets {list(time_offsets)}")
    if len(pi) == 0:
        raise ValueError("No adjacent frame distances found. Dataset may not have tracks with multiple timepoints.")
    ri, rj = random_pairs(x.shape[0], len(pi))
    found = {"adjacent": _pair_dist(z, pi, pj, metric, 0.0), "random": _pair_dist(z, ri, rj, metric, 0.0)}

    stats = {}
    for kind, dist in found.items():      # the reference's key order: the four of the adjacent pairs, then the four of the random ones
        for name, value in (("mean", np.mean(dist)), ("std", np.std(dist)), ("median", np.median(dist)),
                            ("peak", find_distribution_peak(dist, method="kde_robust"))):
            stats[f"{kind}_frame_{name}"] = float(value)
    stats["smoothness_score"] = float(np.mean(found["adjacent"]) / np.mean(found["random"]))
    stats["dynamic_range"] = stats["random_frame_peak"] - stats["adjacent_frame_peak"]
    for key, value in stats.items():
        say(f"  {key} = {value:.6g}")
    per_track = [part.tolist() for part in np.split(found["adjacent"][piecewise], splits)] if len(piecewise) else []
    return stats, {f"{kind}_frame_distribution": dist for kind, dist in found.items()}, per_track


def compute_track_displacement(embedding_dataset, distance_metric="cosine") -> dict[int, list[float]]:
    """Embedding displacement per time lag -> {tau: [distances]}: for every track (first-appearance order of (fov_name, track_id)),
    its rows sorted by t, every pair (i, i + off), off = 1 .. T - 1, ascending i, filed under ``tau = int(t[i + off] - t[i])``; the keys
    are in insertion order.  ``embedding_dataset`` is a mapping with ``"features"``, ``"fov_name"``, ``"track_id"``, ``"t"``.  The
    distances are ``vsx_pair_dist`` on the raw features (cosine with ``F.normalize``'s eps 1e-12: a zero row is at distance 1), in
    calls of at most 2^22 pairs"""
    metric = _metric(distance_metric)
    if not isinstance(embedding_dataset, Mapping):
        raise TypeError("embedding_dataset must be a mapping with 'features', 'fov_name', 'track_id' and 't'")
    x = _features(embedding_dataset["features"])
    t = column(embedding_dataset["t"])
    rows, starts, lengths = track_pairs(embedding_dataset["fov_name"], embedding_dataset["track_id"], t)
    if len(rows) != x.shape[0]:
        raise ValueError(f"the metadata have {len(rows)} rows, the features {x.shape[0]}")
    eps = 1e-12 if metric == "cosine" else 0.0
    parts: dict[int, list[np.ndarray]] = {}
    cache: dict = {}

    def flush(batch_i, batch_j):
        if not batch_i:
            return
        pi, pj = np.concatenate(batch_i), np.concatenate(batch_j)
        dist = _pair_dist(x, pi, pj, metric, eps)
        tau = (t[pj] - t[pi]).astype(np.int64)          # truncates toward zero, as int()
        order = np.argsort(tau, kind="stable")
        cut = np.flatnonzero(np.diff(tau[order])) + 1
        groups = np.split(order, cut)
        for grp in sorted(groups, key=lambda g_: g_[0]):  # a new key enters the dict where it first appears
            parts.setdefault(int(tau[grp[0]]), []).append(dist[grp])

    batch_i, batch_j, held = [], [], 0
    for s, T in zip(starts.tolist(), lengths.tolist()):
        if T < 2:
            continue
        i, j = _offset_major(T, cache)
        if held and held + len(i) > MSD_CHUNK:
            flush(batch_i, batch_j)
            batch_i, batch_j, held = [], [], 0
        batch_i.append(rows[s + i]), batch_j.append(rows[s + j])
        held += len(i)
    flush(batch_i, batch_j)
    return {tau: np.concatenate(v).tolist() for tau, v in parts.items()}
