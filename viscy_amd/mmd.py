"""Maximum mean discrepancy with a Gaussian RBF kernel and its permutation test on the device: the four functions of
``viscy_utils.evaluation.mmd`` (what ``dynaclr evaluate mmd`` runs per marker x condition pair x time bin), with the same names,
keywords, defaults and return types.

The reference materialises the pooled N x N kernel (N = n + m) and multiplies it twice by the (N, P) label matrix.  Here nothing
quadratic is stored: ``vsx_mmd_sums`` (csrc/mmd.hip) streams 128 x 128 tiles of the kernel, formed once each on the exact-fp32
tile engine, against the label tiles and reduces them to three sums per label vector in float64; the workspace is O(N P / 128).

    quad = z'Kz,  zr = z'K1,  T = 1'K1   ->   sum_XX = quad,  sum_XY = zr - quad,  sum_YY = T - 2 zr + quad
    mmd2 = sum_XX / (n (n - 1)) + sum_YY / (m (m - 1)) - 2 sum_XY / (n m)                      (float64)

The pool is centred by its column mean before any distance is formed (squared distances do not change; the fp32 Gram form
``n_i + n_j - 2 dot`` then stays accurate for embeddings far from the origin).  Random draws stay on the host with numpy, draw for
draw as the reference: ``default_rng(0).choice`` for the median heuristic's subsample, ``default_rng(seed).permutation(N)`` once
per permutation, the first ``n`` entries of which form the X group.

Inputs are numpy arrays or torch tensors; a tensor already on the device is used in place.  There is no CPU path: without a HIP
device the functions raise ``RuntimeError``.  The input checks and the device rule are ``evalkit``'s (``as_matrix`` without a row or
column minimum: the two-rows-a-side rule of the unbiased estimate is checked here).

Deliberate differences from the reference:

* values are float64 on return (the reference's null distribution is float32);
* the 20 000-row cap (``_MMD_PERM_MAX_N``) does not apply; the limits are those of ``vsx_mmd_sums`` (N <= 2^24, P <= 2^24);
* ``ValueError`` for ``n < 2`` or ``m < 2`` (the reference divides by zero), for ``n_permutations < 1``, for ``bandwidth <= 0`` and
  for non-finite input ("Input X contains NaN or infinity.", as ``knn_predict``);
* the median heuristic's distances and the kernel's exponent are float32 (centred Gram form), not float64 ``cdist``.
"""

from __future__ import annotations

import numpy as np
import torch
from torch import Tensor

from .evalkit import as_matrix, device_of, to_device

__all__ = ["median_heuristic", "gaussian_rbf_kernel", "compute_mmd_unbiased", "mmd_permutation_test", "permutation_labels"]


def _pair(X, Y):
    X, Y = as_matrix(X, "X"), as_matrix(Y, "Y")
    if X.shape[1] != Y.shape[1]:
        raise ValueError(f"X {tuple(X.shape)} and Y {tuple(Y.shape)} differ in width")
    return X, Y


def _bandwidth(bandwidth) -> float:
    bandwidth = float(bandwidth)
    if not bandwidth > 0.0 or not np.isfinite(bandwidth):
        raise ValueError(f"bandwidth={bandwidth} must be positive and finite")
    return bandwidth


def _device(X, Y) -> torch.device:
    return device_of(X, Y, who="mmd")


def _pool(X, Y, dev: torch.device) -> Tensor:
    return torch.cat((to_device(X, dev), to_device(Y, dev)), dim=0)


def permutation_labels(n: int, m: int, n_permutations: int, seed: int) -> np.ndarray:
    """uint8 (n_permutations + 1, n + m): row 0 labels the first ``n`` pooled rows 1 (the observed split); row 1 + p labels the
    first ``n`` entries of the p-th ``default_rng(seed).permutation(n + m)``, the reference's ``z_null``"""
    N = n + m
    z = np.zeros((n_permutations + 1, N), dtype=np.uint8)
    z[0, :n] = 1
    rng = np.random.default_rng(seed)
    for p in range(n_permutations):
        z[p + 1, rng.permutation(N)[:n]] = 1
    return z


def median_heuristic(X, Y, subsample: int = 1000) -> float:
    """The Gaussian RBF bandwidth sigma^2 by the median heuristic: the median of the pairwise squared distances of (at most
    ``subsample`` rows drawn jointly from) X and Y, plus 1e-12.  The distances are formed on the device (``vsx_sqdist_upper``), the
    one or two middle order statistics are exact (``vsx_row_select``) and averaged in float64."""
    from . import ops
    from .transforms import row_select

    X, Y = _pair(X, Y)
    total = len(X) + len(Y)
    if total < 2 or int(subsample) < 2:
        raise ValueError(f"median_heuristic needs at least two pooled rows (got {total}, subsample={subsample})")
    dev = _device(X, Y)
    pool = _pool(X, Y, dev)
    if total > subsample:
        idx = np.random.default_rng(0).choice(total, subsample, replace=False)
        pool = pool[torch.from_numpy(idx).to(dev)].contiguous()
    xc, norms, _ = ops.mmd_prepare(pool)
    upper = ops.sqdist_upper(xc, norms)
    L = upper.shape[1]
    mid = row_select(upper, ((L - 1) // 2, L // 2)).to(torch.float64).cpu().numpy()[0]
    return float(0.5 * (mid[0] + mid[1])) + 1e-12


def gaussian_rbf_kernel(X, Y, bandwidth: float) -> np.ndarray:
    """K(X, Y) (n, m) float32, ``exp(-||x - y||^2 / (2 bandwidth))``: the rows-of-X x columns-of-Y block of the pooled kernel, with
    the kernel values of ``mmd_permutation_test`` (``vsx_rbf_block``)"""
    from . import ops

    X, Y = _pair(X, Y)
    bandwidth = _bandwidth(bandwidth)
    n, m = len(X), len(Y)
    if n < 1 or m < 1:
        raise ValueError(f"gaussian_rbf_kernel needs rows on both sides (got {n} and {m})")
    dev = _device(X, Y)
    xc, norms, _ = ops.mmd_prepare(_pool(X, Y, dev))
    return ops.rbf_block(xc, norms, (0, n), (n, n + m), bandwidth, False).cpu().numpy()


def _mmd2_of_labels(X, Y, labels: np.ndarray, bandwidth) -> np.ndarray:
    """float64 (P,): MMD^2 of every label vector"""
    from . import ops

    n, m = len(X), len(Y)
    if bandwidth is None:
        bandwidth = median_heuristic(X, Y)
    dev = _device(X, Y)
    xc, norms, _ = ops.mmd_prepare(_pool(X, Y, dev))
    sums = ops.mmd_sums(xc, norms, torch.from_numpy(labels).to(dev), bandwidth).cpu().numpy()
    return sums[:, 0] / (n * (n - 1.0)) + sums[:, 1] / (m * (m - 1.0)) - 2.0 * sums[:, 2] / (float(n) * m)


def _checked(X, Y, bandwidth):
    X, Y = _pair(X, Y)
    if len(X) < 2 or len(Y) < 2:
        raise ValueError(f"the unbiased MMD^2 needs at least two rows on either side (got {len(X)} and {len(Y)})")
    return X, Y, None if bandwidth is None else _bandwidth(bandwidth)


def compute_mmd_unbiased(X, Y, bandwidth: float | None = None) -> float:
    """The unbiased quadratic-time MMD^2 estimate; ``bandwidth`` None = median heuristic.  Bit for bit the observed value of
    ``mmd_permutation_test``."""
    X, Y, bandwidth = _checked(X, Y, bandwidth)
    return float(_mmd2_of_labels(X, Y, permutation_labels(len(X), len(Y), 0, 0), bandwidth)[0])


def mmd_permutation_test(X, Y, n_permutations: int = 1000, bandwidth: float | None = None,
                         seed: int = 42) -> tuple[float, float, np.ndarray]:
    """-> (mmd2, p_value, null_distribution (n_permutations,) float64): the observed unbiased MMD^2, its permutation p-value
    ``(sum(null >= observed) + 1) / (n_permutations + 1)`` and the null values, one kernel pass for all label vectors"""
    X, Y, bandwidth = _checked(X, Y, bandwidth)
    n_permutations = int(n_permutations)
    if n_permutations < 1:
        raise ValueError(f"n_permutations={n_permutations} must be at least 1")
    _device(X, Y)  # refuse before the host draws
    vals = _mmd2_of_labels(X, Y, permutation_labels(len(X), len(Y), n_permutations, seed), bandwidth)
    observed, null = float(vals[0]), vals[1:].copy()
    p_value = float((np.sum(null >= observed) + 1) / (n_permutations + 1))
    return observed, p_value, null
