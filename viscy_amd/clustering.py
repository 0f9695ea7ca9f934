"""Clustering evaluation of embeddings on the device: ``viscy_utils.evaluation.clustering`` with the reference's names, keywords,
defaults and return types.

The reference forms an N x N float64 distance matrix with torch and hands the embeddings to sklearn's ``DBSCAN`` and
``KNeighborsClassifier``.  Here the arithmetic is float64 on the matrix cores (csrc/clustering.hip on the tile engine of
csrc/f64_tile.h: fp32 rows converted where they are staged, every product exact, one summation order):

    vsx_row_sqnorm_f64   the engine's own dot of every row with itself
    vsx_pdist_f64        blocks of the cosine / Euclidean / squared Euclidean distance matrix
    vsx_eps_graph        the eps-neighbourhood graph as a bit matrix, N^2 / 8 bytes instead of 8 N^2, and its row counts
    vsx_cc_round         rounds of minimum-label hooking and pointer jumping over the core-core edges
    vsx_dbscan_finish    cluster numbers for core, border and noise rows
    vsx_knn_vote         (csrc/online_eval.hip) the neighbours' majority vote

DBSCAN's labelling is order-free: a row is core if at least ``min_samples`` rows, itself included, lie within ``eps``; clusters are
the components of the core rows, numbered by their smallest core index; a border row takes the smallest cluster number among its
core neighbours; the rest is noise (-1).  That is what sklearn's scan in index order produces, so the labels are sklearn's wherever
no pair lies within rounding of ``eps``, and they are the same from run to run.  NMI and ARI are restated on the host in float64 and
Python integers.  There is no CPU path for the kernels: without a HIP device the functions raise ``RuntimeError``.  scipy and
sklearn are not imported.  Input handling is ``evalkit``'s.

Deliberate differences from the reference:

* the embeddings are taken as float32 (the reference upcasts float32 to float64 and keeps float64 input as it is);
* the diagonal of a distance matrix is exactly 0 and the matrix is symmetric bit for bit; two bit-identical rows are at Euclidean
  distance exactly 0 (their cosine distance is within rounding of 0, and 1 for two zero rows);
* ``device`` "cpu", ``None`` and "scipy" raise ``RuntimeError`` and a metric other than "cosine" / "euclidean" raises ``ValueError``;
* ``rank_nearest_neighbors`` breaks ties towards the lower index (the reference's quicksort leaves them undefined);
* ``dbscan_clustering`` compares squared float64 distances with ``eps * eps`` (sklearn compares float32 distances for float32 input)
  and refuses a graph above ``MAX_GRAPH_BYTES``;
* ``knn_accuracy`` orders neighbours by (distance, index) and serves ``1 <= k <= VSX_KNN_MAX_K``.
"""

from __future__ import annotations

import math

import numpy as np
import torch

from .evalkit import as_matrix, column, device_of, to_device, upload

__all__ = ["knn_accuracy", "pairwise_distance_matrix", "rank_nearest_neighbors", "select_block", "compare_time_offset",
           "dbscan_clustering", "clustering_evaluation", "normalized_mutual_info", "adjusted_rand", "graph_workspace"]

MAX_GRAPH_BYTES = 16 << 30       # largest bit matrix dbscan_clustering allocates: N ceil(N / 64) 8 bytes, N about 370 000
MAX_MATRIX_BYTES = 2 << 30       # a distance matrix up to this size is filled on the device in one call
BLOCK_BYTES = 256 << 20          # else row blocks of about this size go to a host array; also knn_accuracy's row blocks

_workspaces: dict = {}


# ------------------------------------------------------------------------------------------------ input plumbing
def _features(X, who_name: str = "features") -> torch.Tensor:
    """float32 (N, d) on the device, N >= 1, d >= 1, finite (looked for where the data live); the device is looked for first"""
    dev = device_of(X, who="clustering")
    X = as_matrix(X, who_name, min_cols=1, unwrap=True)
    if X.shape[0] < 1:
        raise ValueError(f"{who_name} needs at least one row")
    return to_device(X, dev)


def _block_rows(n: int, tile: int) -> int:
    """rows of a block of about BLOCK_BYTES of float64 over n columns: a positive multiple of the tile"""
    return max(BLOCK_BYTES // (8 * n) // tile, 1) * tile


def graph_workspace(dev: torch.device, nbytes: int) -> torch.Tensor:
    """the grow-only byte buffer on ``dev`` that ``dbscan_clustering`` carves its graph, counts, labels and flag from; nothing in it
    is read before it is written, so it may hold any contents"""
    key = (dev.type, dev.index)
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < nbytes:
        _workspaces[key] = ws = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
    return ws


# ------------------------------------------------------------------------------------------------ distances and ranks
def pairwise_distance_matrix(features, metric: str = "cosine", device: str = "auto") -> np.ndarray:
    """-> float64 (N, N): cosine (``F.normalize``'s rule: a zero row is at distance 1) or Euclidean distances of all rows, float64
    throughout (``vsx_pdist_f64``): exactly 0 on the diagonal, symmetric bit for bit.  ``device``: "auto", "cuda" or "gpu"; the matrix
    is filled on the device when it fits ``MAX_MATRIX_BYTES``, else in row blocks into the host array"""
    from . import ops

    if metric not in ("cosine", "euclidean"):
        raise ValueError(f"metric {metric!r} is not served on the device: use 'cosine' or 'euclidean'")
    if device in (None, "scipy", "cpu"):
        raise RuntimeError(f"viscy_amd.clustering needs the HIP device (no CPU fallback): device={device!r} is not served")
    if device not in ("auto", "cuda", "gpu"):
        raise ValueError(f"Invalid device: {device}. Use 'auto', 'cuda', 'cpu', or 'scipy'")
    x = _features(features)
    n = int(x.shape[0])
    norms = ops.row_sqnorm_f64(x)
    if 8 * n * n <= MAX_MATRIX_BYTES:
        return ops.pdist_f64(x, norms, metric).cpu().numpy()
    out = np.empty((n, n), dtype=np.float64)
    step = _block_rows(n, ops.F64_TILE)
    for r0 in range(0, n, step):
        r1 = min(r0 + step, n)
        out[r0:r1] = ops.pdist_f64(x, norms, metric, rows=(r0, r1)).cpu().numpy()
    return out


def rank_nearest_neighbors(cross_dissimilarity, normalize: bool = True):
    """Rank every sample by dissimilarity to all others along axis 1: a stable double argsort, ties to the lower index.  An ndarray
    is ranked with numpy and a tensor where it lives; int64, or float64 in [0, 1] when ``normalize``"""
    if torch.is_tensor(cross_dissimilarity):
        order = torch.argsort(cross_dissimilarity.detach(), dim=1, stable=True)
        rankings = torch.argsort(order, dim=1, stable=True)
        if not normalize:
            return rankings
        n = int(rankings.shape[1])      # the n quotients come from the host: a device's float64 division need not round as IEEE's
        with np.errstate(invalid="ignore"):
            fractions = np.arange(n, dtype=np.float64) / np.float64(n - 1)
        return torch.from_numpy(fractions).to(rankings.device)[rankings]
    order = np.argsort(np.asarray(cross_dissimilarity), axis=1, kind="stable")
    rankings = np.argsort(order, axis=1, kind="stable").astype(np.int64)
    return rankings.astype(np.float64) / (rankings.shape[1] - 1) if normalize else rankings


def select_block(distances, index):
    """Select with the same indexes along both dimensions for a square matrix."""
    return distances[index][:, index]


def compare_time_offset(single_track_distances, time_offset: int = 1):
    """The distances / rankings of the sample ``time_offset`` later than each sample: the diagonal ``-time_offset``, (n - offset,)"""
    return single_track_distances.diagonal(offset=-time_offset)


# ------------------------------------------------------------------------------------------------ DBSCAN
def dbscan_clustering(embeddings, eps=0.5, min_samples=5) -> np.ndarray:
    """-> int64 (N,): sklearn's ``DBSCAN(eps, min_samples).fit_predict`` labels (-1 = noise) from the bit graph of
    ``d2_ij <= eps * eps`` (``vsx_eps_graph``), components of the core rows by rounds of ``vsx_cc_round`` until nothing changes (at
    most N + 1: more is a ``RuntimeError``) and ``vsx_dbscan_finish``.  The graph takes ``N ceil(N / 64) 8`` bytes; above
    ``MAX_GRAPH_BYTES`` this raises ``ValueError`` before any launch"""
    from . import ops

    eps, min_samples = float(eps), int(min_samples)
    if not (eps > 0.0 and math.isfinite(eps)):
        raise ValueError(f"eps={eps} must be a positive finite number")
    if min_samples < 1:
        raise ValueError(f"min_samples={min_samples} must be at least 1")
    X = embeddings
    n_rows = int(X.shape[0]) if hasattr(X, "shape") and len(X.shape) == 2 else len(X)
    words = ops.eps_graph_words(n_rows)
    graph_bytes = n_rows * words * 8
    if graph_bytes > MAX_GRAPH_BYTES:
        raise ValueError(f"the neighbourhood graph of {n_rows} rows takes {graph_bytes} bytes, above MAX_GRAPH_BYTES = {MAX_GRAPH_BYTES}")
    x = _features(X, "embeddings")
    n, dev = int(x.shape[0]), x.device
    ws = graph_workspace(dev, graph_bytes + 4 * (3 * n + 1))
    adj = ws[:graph_bytes].view(torch.int64).view(n, words)
    ints = ws[graph_bytes:graph_bytes + 4 * (3 * n + 1)].view(torch.int32)
    deg, labels, out, changed = ints[:n], ints[n:2 * n], ints[2 * n:3 * n], ints[3 * n:]

    norms = ops.row_sqnorm_f64(x)
    ops.eps_graph(x, norms, eps * eps, adj, deg)
    core = (deg >= min_samples).to(torch.uint8)
    index = torch.arange(n, dtype=torch.int32, device=dev)
    labels.copy_(index)
    for _ in range(n + 1):
        ops.cc_round(adj, core, labels, changed)
        if int(changed.item()) == 0:
            break
    else:
        raise RuntimeError(f"dbscan_clustering: the components of {n} rows did not settle in {n + 1} rounds")
    roots = (core.bool() & (labels == index)).to(torch.int32)
    cid = (torch.cumsum(roots, 0) - roots).to(torch.int32)
    return ops.dbscan_finish(adj, core, labels, cid, out).cpu().numpy().astype(np.int64)


# ------------------------------------------------------------------------------------------------ NMI / ARI on the host
def _contingency(labels_true, labels_pred) -> np.ndarray:
    a, b = column(labels_true).reshape(-1), column(labels_pred).reshape(-1)
    if len(a) != len(b):
        raise ValueError(f"labels_true has {len(a)} entries, labels_pred {len(b)}")
    ca, ia = np.unique(a, return_inverse=True)
    cb, ib = np.unique(b, return_inverse=True)
    table = np.zeros((len(ca), len(cb)), dtype=np.int64)
    np.add.at(table, (ia.reshape(-1), ib.reshape(-1)), 1)
    return table


def _entropy(counts: np.ndarray) -> float:
    pi = counts[counts > 0].astype(np.int64)
    if pi.size <= 1:
        return 0.0
    total = pi.sum()
    return float(-np.sum((pi / total) * (np.log(pi) - math.log(total))))


def normalized_mutual_info(labels_true, labels_pred) -> float:
    """sklearn's ``normalized_mutual_info_score``: natural logarithms, the arithmetic mean of the two entropies, 1.0 when both
    labelings have one class (or no entry), 0.0 for a mutual information below float64's epsilon"""
    table = _contingency(labels_true, labels_pred)
    if table.shape[0] == table.shape[1] == 1 or table.size == 0:
        return 1.0
    nzx, nzy = np.nonzero(table)
    nz = table[nzx, nzy]
    total = table.sum()
    pi, pj = table.sum(axis=1), table.sum(axis=0)
    frac = nz / total
    log_outer = -np.log(pi[nzx] * pj[nzy]) + math.log(pi.sum()) + math.log(pj.sum())
    terms = frac * (np.log(nz) - math.log(total)) + frac * log_outer
    terms = np.where(np.abs(terms) < np.finfo(np.float64).eps, 0.0, terms)
    mi = float(np.clip(terms.sum(), 0.0, None))
    if abs(mi) < np.finfo(np.float64).eps:
        return 0.0
    return float(mi / (0.5 * (_entropy(pi) + _entropy(pj))))


def adjusted_rand(labels_true, labels_pred) -> float:
    """sklearn's ``adjusted_rand_score`` from the pair counts as Python integers; 1.0 when ``fp == fn == 0``"""
    table = _contingency(labels_true, labels_pred)
    n = int(table.sum())
    squares = sum(int(v) ** 2 for v in table.reshape(-1))
    tp = squares - n
    fp = sum(int(v) ** 2 for v in table.sum(axis=0)) - squares
    fn = sum(int(v) ** 2 for v in table.sum(axis=1)) - squares
    tn = n * n - fp - fn - squares
    if fn == 0 and fp == 0:
        return 1.0
    return float(2.0 * (tp * tn - fn * fp) / ((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn)))


def clustering_evaluation(embeddings, annotations, method="nmi") -> float:
    """DBSCAN with its defaults, scored against ``annotations`` by NMI or ARI"""
    if method not in ("nmi", "ari"):
        raise ValueError("Invalid method. Choose 'nmi' or 'ari'.")
    clusters = dbscan_clustering(embeddings)
    return normalized_mutual_info(annotations, clusters) if method == "nmi" else adjusted_rand(annotations, clusters)


# ------------------------------------------------------------------------------------------------ k-NN accuracy
def knn_accuracy(embeddings, annotations, k=5) -> float:
    """The accuracy of sklearn's ``KNeighborsClassifier(n_neighbors=k)`` fitted and scored on the same rows: Euclidean, the row
    itself among its neighbours, neighbours in the total order (squared distance ascending, then index ascending: row blocks of
    ``vsx_pdist_f64`` and a stable sort), the majority vote of ``vsx_knn_vote`` over class codes from a sorted ``np.unique`` (ties to
    the smallest class)"""
    from . import ops

    k = int(k)
    if not 1 <= k <= ops.KNN_MAX_K:
        raise ValueError(f"k={k} must be in [1, {ops.KNN_MAX_K}]")
    x = _features(embeddings, "embeddings")
    n = int(x.shape[0])
    if k > n:
        raise ValueError(f"Expected n_neighbors <= n_samples_fit, but n_neighbors = {k}, n_samples_fit = {n}")
    y = column(annotations).reshape(-1)
    if len(y) != n:
        raise ValueError(f"annotations has {len(y)} entries, embeddings {n} rows")
    _, codes = np.unique(y, return_inverse=True)
    codes_d = upload(codes.reshape(-1), x.device, np.int32)
    norms = ops.row_sqnorm_f64(x)
    idx = torch.empty((n, k), dtype=torch.int32, device=x.device)
    step = _block_rows(n, ops.F64_TILE)
    for r0 in range(0, n, step):
        r1 = min(r0 + step, n)
        d2 = ops.pdist_f64(x, norms, "sqeuclidean", rows=(r0, r1))
        idx[r0:r1] = torch.sort(d2, dim=1, stable=True).indices[:, :k].to(torch.int32)
    cnt = torch.full((n,), k, dtype=torch.int32, device=x.device)
    pred = ops.knn_vote(idx, cnt, codes_d)
    return float((pred == codes_d).sum().item() / n)
