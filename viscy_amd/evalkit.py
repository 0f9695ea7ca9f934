"""The host layer under the evaluation modules (``reduce``, ``linear_classifier``, ``mmd``, ``smoothness``, ``clustering``, ``online_eval``): what an
entry point does with its arguments before a kernel sees them, and the rules of sklearn that more than one module restates.  Pure
numpy / torch; nothing here loads the kernel library.

Inputs are numpy arrays or torch tensors.  ``as_matrix`` checks one where it lives, ``device_of`` picks the device (there is no CPU
path: without a HIP device it raises ``RuntimeError``), ``to_device`` / ``upload`` put data there, and ``padded_to_two_rows`` serves
the single row that the kernels (n >= 2) do not.  A new evaluation entry point takes its input handling from here.
"""

from __future__ import annotations

import numpy as np
import torch
from torch import Tensor

__all__ = ["device_of", "as_matrix", "to_device", "column", "upload", "padded_to_two_rows", "approximate_mode",
           "stratified_shuffle_parts", "average_ranks"]


# ------------------------------------------------------------------------------------------------ inputs
def device_of(*arrays, who: str) -> torch.device:
    """the device of the first tensor that is on one, else the current device; ``who`` is the module that asks"""
    for a in arrays:
        if torch.is_tensor(a) and a.is_cuda:
            return a.device
    if not torch.cuda.is_available():
        raise RuntimeError(f"viscy_amd.{who} needs the HIP device (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def as_matrix(X, name: str = "X", *, min_rows: int = 0, min_cols: int = 0, width: int | None = None, finite: bool = True,
              unwrap: bool = False):
    """-> the detached tensor or the ndarray, a (rows, d) matrix.  ``ValueError`` in this order: not 2-D, fewer than ``min_rows``
    (0 or 2) rows, fewer than ``min_cols`` (0 or 1) columns, not ``width`` columns (the width an estimator was fitted with; this
    message also answers a wrong dimension), a value that is not finite (sklearn's message; looked for where the data live).
    ``unwrap`` takes the ``.values`` of a pandas / xarray object."""
    if torch.is_tensor(X):
        X = X.detach()
    else:
        X = np.asarray(getattr(X, "values", X) if unwrap else X)
    if width is not None:
        if X.ndim != 2 or X.shape[1] != width:
            raise ValueError(f"{name} {tuple(X.shape)} must be (rows, {width})")
    elif X.ndim != 2:
        raise ValueError(f"{name} must be a (rows, d) matrix, got {tuple(X.shape)}")
    if X.shape[0] < min_rows:
        raise ValueError(f"{name} needs at least two rows (got {X.shape[0]})")
    if X.shape[1] < min_cols:
        raise ValueError(f"{name} needs at least one feature")
    if finite and not bool((torch.isfinite(X) if torch.is_tensor(X) else np.isfinite(X)).all()):
        raise ValueError("Input X contains NaN or infinity.")
    return X


def to_device(X, dev: torch.device) -> Tensor:
    """float32, contiguous, on ``dev``; a tensor that already is all three is returned as it is"""
    t = X if torch.is_tensor(X) else torch.from_numpy(np.array(X, dtype=np.float32))  # a copy: the caller's array may be read-only
    return t.to(device=dev, dtype=torch.float32).contiguous()


def column(v) -> np.ndarray:
    """a metadata column (a tensor, a pandas column, an array or a list) as an ndarray"""
    if torch.is_tensor(v):
        return v.detach().cpu().numpy()
    return np.asarray(getattr(v, "values", v))


def upload(a, dev: torch.device, dtype=None) -> Tensor:
    """a host array as a contiguous tensor of ``dtype`` (the array's own by default) on ``dev``: the int32 pair and label lists, the
    float64 moment and weight vectors"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)


def padded_to_two_rows(x: Tensor) -> tuple[Tensor, int]:
    """-> (x2, n_rows): the kernels serve n >= 2, so a single row rides with a copy of itself and the caller keeps ``[:n_rows]`` of
    the result; any other ``x`` is returned as it is"""
    n = int(x.shape[0])
    return (torch.cat((x, x)) if n == 1 else x), n


# ------------------------------------------------------------------------------------------------ sklearn's rules, restated once
def approximate_mode(class_counts: np.ndarray, n_draws: int, rng: np.random.RandomState) -> np.ndarray:
    """sklearn.utils.extmath._approximate_mode: proportional allocation, remainders by size, exact ties by ``rng.choice``"""
    continuous = class_counts / class_counts.sum() * n_draws
    floored = np.floor(continuous)
    need = int(n_draws - floored.sum())
    if need > 0:
        remainder = continuous - floored
        for value in np.sort(np.unique(remainder))[::-1]:
            (inds,) = np.where(remainder == value)
            add = min(len(inds), need)
            inds = rng.choice(inds, size=add, replace=False)
            floored[inds] += 1
            need -= add
            if need == 0:
                break
    return floored.astype(int)


def stratified_shuffle_parts(y, n_train: int, n_test: int, rng: np.random.RandomState) -> tuple[list, list]:
    """One draw of sklearn's ``StratifiedShuffleSplit`` -> (train, test) row indices as lists, class by class in ``np.unique`` order:
    the rows of a class by mergesort, the class allocations of the train part and then of the test part by ``approximate_mode``,
    then one ``rng.permutation`` per class, whose first entries are the class's train rows and the next its test rows.  numpy's
    legacy ``RandomState`` stream is frozen, so the restatement draws what sklearn draws; ``rng`` is left where sklearn's closing
    permutations of the two parts would start.  The callers check the sizes (at least one row per class and part)."""
    _, y_idx = np.unique(np.asarray(y), return_inverse=True)
    y_idx = y_idx.reshape(-1)
    counts = np.bincount(y_idx)
    class_indices = np.split(np.argsort(y_idx, kind="mergesort"), np.cumsum(counts)[:-1])
    n_i = approximate_mode(counts, n_train, rng)
    t_i = approximate_mode(counts - n_i, n_test, rng)
    train, test = [], []
    for c in range(len(counts)):
        perm = class_indices[c].take(rng.permutation(counts[c]), mode="clip")
        train.extend(perm[: n_i[c]])
        test.extend(perm[n_i[c]: n_i[c] + t_i[c]])
    return train, test


def average_ranks(t):
    """tie-averaged ranks 1 .. n as ``scipy.stats.rankdata`` (float64); a torch tensor is ranked on its device (sort +
    ``unique_consecutive``), anything else with numpy"""
    if torch.is_tensor(t):
        v, order = torch.sort(t.reshape(-1))
        _, inverse, counts = torch.unique_consecutive(v, return_inverse=True, return_counts=True)
        last = torch.cumsum(counts, 0).to(torch.float64)
        avg = last - (counts.to(torch.float64) - 1.0) / 2.0
        ranks = torch.empty(v.numel(), dtype=torch.float64, device=t.device)
        ranks[order] = avg[inverse]
        return ranks
    a = np.asarray(t).reshape(-1)
    order = np.argsort(a, kind="stable")
    v = a[order]
    new = np.concatenate(([True], v[1:] != v[:-1]))
    inverse = np.cumsum(new) - 1
    counts = np.bincount(inverse)
    avg = np.cumsum(counts) - (counts - 1) / 2.0
    ranks = np.empty(len(a), dtype=np.float64)
    ranks[order] = avg[inverse]
    return ranks
