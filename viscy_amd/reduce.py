"""PCA on the device: ``compute_pca`` of ``viscy_utils.evaluation.dimensionality_reduction`` (what ``dynaclr evaluate reduce``,
``EmbeddingWriter``, ``pca_pairplot`` and ``LinearClassifierPipeline(use_pca=True)`` call), with the same name, keywords, defaults
and return types, and the two sklearn estimators under it, ``StandardScaler`` and ``PCA``, with sklearn's attribute names.

The route is sklearn's ``covariance_eigh``.  The embeddings (N = 10^5 .. 10^6 rows x 768) are read three times on the device
(csrc/pca.hip) and nothing N-sized but the projection is written:

    vsx_col_moments     mean, sum (x - mean)^2                      float64, fixed-order folds
    vsx_gram_centered   G = (X - mean)' (X - mean)  (d, d)          fp32 MFMA over blocks of 128 rows, float64 past the block
    vsx_center_project  Z = (X - mean) W'            (N, k)         fp32, the dots of csrc/f32_tile.h

Everything between the second and the third is a d x d problem on the host, in float64, in one pure function
(``pca_from_moments``): the standard scaling of G (``G_ij / (s_i s_j)``, never a pass over the data), ``numpy.linalg.eigh``, the
descending order, the clip of negative eigenvalues, ``svd_flip(u_based_decision=False)`` and the attributes.  ``1 / scale`` is
folded into W, so one projection kernel serves both ``normalize_features`` settings.

Inputs are numpy arrays or torch tensors; a tensor already on the device is used in place.  A mapping with ``"features"`` and any of
``"id"``, ``"fov_name"``, ``"t"``, ``"track_id"`` stands in for the reference's xarray ``Dataset``.  There is no CPU path for the data
passes: without a HIP device ``fit`` / ``transform`` / ``compute_pca`` raise ``RuntimeError``.  The checks, the device rule and the
uploads are ``evalkit``'s; ``project`` and ``served`` are what ``linear_classifier`` shares with the estimators here.

Deliberate differences from sklearn:

* moments, covariance and spectrum are float64 whatever the input type (sklearn stays in float32 for float32 input); the
  projection is float32;
* the mean of the standardised data is taken as exactly 0 (sklearn's ``PCA.mean_`` holds its float round-off);
* the solver is always the covariance route (sklearn switches to randomized SVD for small ``n_components`` at d > 500), so
  ``random_state`` is accepted and unused;
* components whose eigenvalue is 0 (N <= D, constant columns) are an arbitrary orthonormal completion;
* ``n_components="mle"`` raises ``NotImplementedError``, and so does d > 4096.
"""

from __future__ import annotations

from collections.abc import Mapping
from dataclasses import dataclass

import numpy as np
import torch
from torch import Tensor

from . import _lib as L
from .evalkit import as_matrix, column, device_of, padded_to_two_rows, to_device, upload

__all__ = ["compute_pca", "StandardScaler", "PCA", "pca_from_moments", "scale_from_moments", "PcaFit", "project", "served"]

MAX_FEATURES = L.PCA_MAX_D  # largest d the PCA and logistic-regression kernels serve
META_COLUMNS = ("id", "fov_name", "t", "track_id")  # the reference's pca_dict order


# ------------------------------------------------------------------------------------------------ host: pure functions
def scale_from_moments(n: int, mean64, m2_64) -> tuple[np.ndarray, np.ndarray]:
    """-> (var_, scale_) of sklearn's StandardScaler: variance with ddof 0; a column ``_is_constant_feature`` calls constant (its
    variance within the two-pass algorithm's error bound ``n eps var + (n mean eps)^2``) gets scale 1"""
    mean64, m2_64 = np.asarray(mean64, dtype=np.float64), np.asarray(m2_64, dtype=np.float64)
    var = m2_64 / float(n)
    eps = np.finfo(np.float64).eps
    constant = var <= n * eps * var + (n * mean64 * eps) ** 2
    scale = np.sqrt(var)
    scale[constant] = 1.0
    scale[scale == 0.0] = 1.0
    return var, scale


def _resolve_components(n_components, n: int, d: int):
    """the checks of sklearn's PCA that need no data: -> None, an int in [1, min(n, d)] or a float in (0, 1)"""
    if isinstance(n_components, str):
        if n_components == "mle":
            raise NotImplementedError("n_components='mle' is not built (the covariance route serves None, an int or a fraction)")
        raise ValueError(f"n_components={n_components!r} must be None, an int or a float in (0, 1)")
    if n_components is None:
        return None
    if isinstance(n_components, (bool, np.bool_)):
        raise ValueError(f"n_components={n_components!r} must be None, an int or a float in (0, 1)")
    if isinstance(n_components, (int, np.integer)):
        if not 1 <= int(n_components) <= min(n, d):
            raise ValueError(f"n_components={n_components} must be between 1 and min(n_samples, n_features)={min(n, d)}")
        return int(n_components)
    if isinstance(n_components, (float, np.floating)) and 0.0 < float(n_components) < 1.0:
        return float(n_components)
    raise ValueError(f"n_components={n_components!r} must be between 1 and min(n_samples, n_features)={min(n, d)}, or a float in (0, 1)")


@dataclass
class PcaFit:
    """what ``pca_from_moments`` answers: sklearn's fitted attributes, and the scaler's next to them"""
    n_samples: int
    data_mean: np.ndarray          # the column mean of the data (StandardScaler.mean_)
    var: np.ndarray                # ddof 0 (StandardScaler.var_)
    scale: np.ndarray              # StandardScaler.scale_; ones without normalize_features
    mean_: np.ndarray              # PCA.mean_: zeros for standardised data, else the data mean
    components_: np.ndarray
    explained_variance_: np.ndarray
    explained_variance_ratio_: np.ndarray
    singular_values_: np.ndarray
    n_components_: int
    noise_variance_: float

    def projection_weights(self) -> np.ndarray:
        """float32 (k, d): components_ / scale, the W of ``vsx_center_project``"""
        return np.ascontiguousarray((self.components_ / self.scale[None, :]).astype(np.float32))


def pca_from_moments(n: int, mean64, m2_64, gram64, n_components=None, normalize_features: bool = True) -> PcaFit:
    """The host part of the fit, float64 throughout, a pure function of the device's three results: covariance
    ``G / (n - 1)`` (of the standardised data: ``G_ij / (s_i s_j)``), ``eigh``, descending order, negative eigenvalues clipped to
    0, ``svd_flip(u_based_decision=False)`` (the entry of largest magnitude of each component is positive), sklearn's
    ``n_components`` rules and attributes"""
    n = int(n)
    mean64 = np.asarray(mean64, dtype=np.float64)
    gram64 = np.asarray(gram64, dtype=np.float64)
    d = mean64.shape[0]
    if gram64.shape != (d, d):
        raise ValueError(f"gram64 {gram64.shape} must be ({d}, {d})")
    if n < 2:
        raise ValueError(f"PCA needs at least two rows (got {n})")
    k = _resolve_components(n_components, n, d)
    var, scale = scale_from_moments(n, mean64, m2_64)
    if not normalize_features:
        scale = np.ones(d)
    C = gram64 / scale[:, None] / scale[None, :] / float(n - 1)
    C = 0.5 * (C + C.T)  # exact for a symmetric G; keeps eigh's one-triangle read honest for any caller
    evals, evecs = np.linalg.eigh(C)
    evals, evecs = evals[::-1].copy(), evecs[:, ::-1]
    evals[evals < 0.0] = 0.0
    Vt = evecs.T.copy()
    big = np.argmax(np.abs(Vt), axis=1)
    signs = np.sign(Vt[np.arange(d), big])
    signs[signs == 0.0] = 1.0
    Vt *= signs[:, None]
    total = evals.sum()
    ratio = evals / total
    sv = np.sqrt(evals * (n - 1))
    if k is None:
        k = min(n, d)
    elif isinstance(k, float):
        k = int(np.searchsorted(np.cumsum(ratio), k, side="right")) + 1
    noise = float(evals[k:].mean()) if k < min(n, d) else 0.0
    return PcaFit(n_samples=n, data_mean=mean64.copy(), var=var, scale=scale,
                  mean_=np.zeros(d) if normalize_features else mean64.copy(), components_=np.ascontiguousarray(Vt[:k]),
                  explained_variance_=evals[:k].copy(), explained_variance_ratio_=ratio[:k].copy(), singular_values_=sv[:k].copy(),
                  n_components_=int(k), noise_variance_=noise)


# ------------------------------------------------------------------------------------------------ what the estimators share
def served(d: int) -> None:
    """``NotImplementedError`` for more features than the PCA and logistic-regression kernels serve"""
    if d > MAX_FEATURES:
        raise NotImplementedError(f"d={d} features: the PCA kernels serve d <= {MAX_FEATURES}")


def project(x: Tensor, mean64: np.ndarray, w32: np.ndarray) -> Tensor:
    """``vsx_center_project``: (x - mean64) w32', float32 on x's device"""
    from . import ops

    return ops.center_project(x, upload(mean64, x.device), upload(w32, x.device))


# ------------------------------------------------------------------------------------------------ estimators
class StandardScaler:
    """sklearn.preprocessing.StandardScaler (with_mean, with_std): ``mean_``, ``var_`` (ddof 0), ``scale_``, ``n_samples_seen_``
    from ``vsx_col_moments``; ``transform`` is ``vsx_center_project`` with the diagonal ``1 / scale_`` and returns float32"""

    def fit(self, X, y=None):
        from . import ops

        X = as_matrix(X, min_rows=2, min_cols=1)
        served(X.shape[1])
        x = to_device(X, device_of(X, who="reduce"))
        mean, m2 = ops.col_moments(x)
        self.mean_ = mean.cpu().numpy()
        self.var_, self.scale_ = scale_from_moments(x.shape[0], self.mean_, m2.cpu().numpy())
        self.n_samples_seen_ = int(x.shape[0])
        self.n_features_in_ = int(x.shape[1])
        return self

    def _check(self, X):
        if not hasattr(self, "scale_"):
            raise RuntimeError("this StandardScaler is not fitted yet")
        return as_matrix(X, width=self.n_features_in_, finite=False)

    def projection_weights(self) -> np.ndarray:
        """float32 (d, d): the diagonal ``1 / scale_``, the W of ``vsx_center_project``"""
        return np.ascontiguousarray(np.diag(1.0 / self.scale_).astype(np.float32))

    def transform(self, X) -> np.ndarray:
        X = self._check(X)
        x, n = padded_to_two_rows(to_device(X, device_of(X, who="reduce")))
        return project(x, self.mean_, self.projection_weights()).cpu().numpy()[:n]

    def fit_transform(self, X, y=None) -> np.ndarray:
        return self.fit(X).transform(X)


class PCA:
    """sklearn.decomposition.PCA on the covariance route: ``components_``, ``explained_variance_``,
    ``explained_variance_ratio_``, ``singular_values_``, ``mean_``, ``n_components_``, ``noise_variance_`` (float64);
    ``transform`` / ``fit_transform`` return float32.  ``normalize_features=True`` fits the standardised data
    (``StandardScaler`` -> ``PCA`` in one pass; ``mean_`` is then that of the standardised data, zero, and ``scaler_`` holds the
    scaler's attributes).  ``random_state`` is accepted and unused: the route is exact."""

    def __init__(self, n_components=None, *, normalize_features: bool = False, random_state=None):
        self.n_components = n_components
        self.normalize_features = bool(normalize_features)
        self.random_state = random_state

    def _fit(self, X):
        from . import ops

        X = as_matrix(X, min_rows=2, min_cols=1)
        _resolve_components(self.n_components, X.shape[0], X.shape[1])
        served(X.shape[1])
        x = to_device(X, device_of(X, who="reduce"))
        mean, m2 = ops.col_moments(x)
        gram = ops.gram_centered(x, mean)
        fit = pca_from_moments(x.shape[0], mean.cpu().numpy(), m2.cpu().numpy(), gram.cpu().numpy(), self.n_components,
                               self.normalize_features)
        self.fit_ = fit
        for name in ("mean_", "components_", "explained_variance_", "explained_variance_ratio_", "singular_values_", "n_components_",
                     "noise_variance_"):
            setattr(self, name, getattr(fit, name))
        self.n_samples_ = fit.n_samples
        self.n_features_in_ = int(x.shape[1])
        if self.normalize_features:
            sc = StandardScaler()
            sc.mean_, sc.var_, sc.scale_, sc.n_samples_seen_, sc.n_features_in_ = fit.data_mean, fit.var, fit.scale, fit.n_samples, self.n_features_in_
            self.scaler_ = sc
        return x

    def fit(self, X, y=None):
        self._fit(X)
        return self

    def _transform(self, x: Tensor) -> np.ndarray:
        return project(x, self.fit_.data_mean, self.fit_.projection_weights()).cpu().numpy()

    def transform(self, X) -> np.ndarray:
        if not hasattr(self, "fit_"):
            raise RuntimeError("this PCA is not fitted yet")
        X = as_matrix(X, width=self.n_features_in_, finite=False)
        x, n = padded_to_two_rows(to_device(X, device_of(X, who="reduce")))
        return self._transform(x)[:n]

    def fit_transform(self, X, y=None) -> np.ndarray:
        return self._transform(self._fit(X))


# ------------------------------------------------------------------------------------------------ the reference's function
def compute_pca(embedding_dataset, n_components=None, normalize_features=True):
    """-> (pc_features float32 ndarray (N, k), pca_df pandas.DataFrame): the reference's ``compute_pca``.  ``embedding_dataset`` is
    an (N, D) numpy array or tensor, or a mapping with ``"features"`` and any of ``"id"``, ``"fov_name"``, ``"t"``, ``"track_id"``
    (they come first in the frame, in that order), then ``PC1`` .. ``PCk``"""
    import pandas as pd

    if isinstance(embedding_dataset, Mapping):
        features = embedding_dataset["features"]
        pca_dict = {c: column(embedding_dataset[c]) for c in META_COLUMNS if c in embedding_dataset}
    else:
        features, pca_dict = embedding_dataset, {}
    features = getattr(features, "values", features) if not torch.is_tensor(features) else features
    pc_features = PCA(n_components=n_components, normalize_features=bool(normalize_features), random_state=42).fit_transform(features)
    for i in range(pc_features.shape[1]):
        pca_dict[f"PC{i + 1}"] = pc_features[:, i]
    return pc_features, pd.DataFrame(pca_dict)

