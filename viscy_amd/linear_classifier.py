"""Linear classifiers on frozen embeddings, on the device: ``viscy_utils.evaluation.linear_classifier`` (what
``dynaclr/evaluation/linear_classifiers`` calls once per task x channel x fold) with the same names, keywords and return values,
and the sklearn estimator under it, ``LogisticRegression``, with sklearn's keywords and fitted attributes.

With n >> d a Newton iteration on the logistic objective is three streaming passes over X (n = 10^5 .. 10^6 rows x 768) and a
(d + 1)^2 Cholesky on the host:

    vsx_logreg_rows   margins, loss, r = dloss/dz, s = d2loss/dz2, q = fl32(sqrt(s))   float64, one wave per row
    vsx_wcolsum       X'r (gradient) and X's (intercept column of the Hessian)            float64, X read once for both
    vsx_gram_scaled   (qX)'(qX) = X' diag(s) X                                            vsx_gram_centered's fp32 MFMA Gram

``newton_fit`` is the host driver, float64, a pure function of a callable that evaluates the data term; the device evaluator is
the three passes, the tests pass a numpy one.  The Gram's fp32 rounding only perturbs the Newton direction: the optimum is fixed
by the float64 gradient, and the iteration stops on it.

Objectives served (``penalty="l2"``, ``dual=False``):

* ``solver="liblinear"``: liblinear's primal ``1/2 |[w; w_b]|^2 + sum_i c_i log(1 + exp(-y_i z_i))``, ``z = x.w + S w_b`` with
  ``S = intercept_scaling``, ``intercept_ = S w_b``.  Two classes (a, b): positive class b, ``cp = C weight_b``,
  ``cn = C weight_a``.  More: one-vs-rest, for class k ``cp = C weight_k`` and ``cn = C`` (liblinear does not weight the rest
  class); ``predict_proba`` is the sigmoid, row-normalised.
* any other sklearn solver name, two classes: the same loss with an unpenalised intercept (those solvers share one optimum).
* multinomial (more than two classes with another solver), ``sample_weight``, other penalties and ``l1_ratio`` raise
  ``NotImplementedError``.

Deliberate differences from sklearn: the fit stops at ``|g| <= eps |g(0)|`` with ``eps = min(tol min(n_pos, n_neg) / n, 1e-10)``,
i.e. at the optimum to float64, whatever ``tol`` (liblinear's own rule with ``tol`` leaves 1e-3-size coefficient errors);
``n_iter_`` counts Newton iterations; ``decision_function`` and the probabilities are float64; there is no CPU path for the data
passes (``RuntimeError`` without a HIP device); d > 4096 raises ``NotImplementedError``.

Input checks, the device rule, the single-row rule and the shared draw of the stratified split are ``evalkit``'s; the projection
kernel's wrapper and the width limit are ``reduce.project`` / ``reduce.served``.

``adata`` is duck-typed (``.X``, ``.obs`` DataFrame, and ``.obsm`` / ``.uns`` mappings for predict).  ``load_and_combine_datasets``
and the two wandb functions of the reference module are not here: they are anndata / wandb plumbing.
"""

from __future__ import annotations

import logging
import warnings
from dataclasses import dataclass
from typing import Any

import numpy as np
import torch
from torch import Tensor

from .evalkit import as_matrix, average_ranks, device_of, padded_to_two_rows, stratified_shuffle_parts, to_device, upload
from .reduce import PCA, StandardScaler, project, served

__all__ = ["LogisticRegression", "LinearClassifierPipeline", "train_linear_classifier", "predict_with_classifier", "newton_fit",
           "NewtonResult", "class_weights", "stratified_split", "group_shuffle_split", "classification_report", "roc_auc"]

_logger = logging.getLogger("viscy_amd")

SOLVERS = ("lbfgs", "liblinear", "newton-cg", "newton-cholesky", "sag", "saga")
ARMIJO = 1e-4        # sufficient-decrease constant
MAX_HALVINGS = 40


# ------------------------------------------------------------------------------------------------ the solver (host, float64)
@dataclass
class NewtonResult:
    w: np.ndarray          # (d,)
    b: float               # the intercept of z = x.w + b (intercept_scaling times the penalised extra weight)
    n_iter: int            # Newton iterations
    n_evals: int           # objective evaluations of the line searches (one row pass each)
    converged: bool
    grad_norm: float       # |g| at (w, b), in the coordinates [w; w_b]
    grad_norm0: float      # |g| at 0


def newton_fit(evaluate, d: int, penalised_intercept: bool = True, intercept_scaling: float = 1.0, tol: float = 1e-10,
               max_iter: int = 100, fit_intercept: bool = True) -> NewtonResult:
    """Damped Newton on ``1/2 |u|_P^2 + data(w, b)`` over ``u = [w; w_b]``, ``b = S w_b``; ``P`` is the identity, with 0 for
    ``w_b`` where the intercept is not penalised (then S = 1).  ``evaluate(w, b, want_hessian)`` answers the data term in
    float64: ``(sum loss, g = X'r (d,), g_b = sum r, G = X' diag(s) X (d, d), h_b = X's (d,), sum s)``; with
    ``want_hessian=False`` only the first entry is read (a line-search trial).  Each iteration solves
    ``(P + [[G, S h_b], [S h_b', S^2 sum s]]) p = -g`` by Cholesky and backtracks on the objective (Armijo).  It stops at
    ``|g| <= tol |g(0)|``, when no step decreases the objective, or after ``max_iter`` iterations (with a warning)."""
    S = float(intercept_scaling) if penalised_intercept else 1.0
    pb = 1.0 if penalised_intercept else 0.0
    k = d + int(bool(fit_intercept))
    pen = np.ones(k)
    if fit_intercept:
        pen[d] = pb

    def split(u):
        return u[:d], (S * float(u[d]) if fit_intercept else 0.0)

    def objective(u):
        return 0.5 * float(pen @ (u * u)) + float(evaluate(*split(u), False)[0])

    def full(u):
        loss, g, g_b, G, h_b, ss = evaluate(*split(u), True)
        grad = pen * u
        grad[:d] += np.asarray(g, dtype=np.float64)
        H = np.zeros((k, k))
        H[:d, :d] = np.asarray(G, dtype=np.float64)
        if fit_intercept:
            grad[d] += S * float(g_b)
            H[:d, d] = H[d, :d] = S * np.asarray(h_b, dtype=np.float64)
            H[d, d] = S * S * float(ss)
        H[np.arange(k), np.arange(k)] += pen
        return 0.5 * float(pen @ (u * u)) + float(loss), grad, H

    u = np.zeros(k)
    f, grad, H = full(u)
    gnorm0 = gnorm = float(np.linalg.norm(grad))
    n_iter = n_evals = 0
    converged = gnorm0 == 0.0
    while not converged and n_iter < max_iter:
        p = _cholesky_solve(H, -grad)
        slope = float(grad @ p)
        # the decrease near the optimum is below the resolution of f: the slack lets a full step through there, and the gradient
        # norm decides below whether it was one
        slack = 8.0 * np.finfo(np.float64).eps * abs(f)
        t, accepted = 1.0, False
        for _ in range(MAX_HALVINGS):
            f_new = objective(u + t * p)
            n_evals += 1
            if f_new <= f + ARMIJO * t * slope + slack:
                accepted = True
                break
            t *= 0.5
        if not accepted:
            break
        u_new = u + t * p
        f_new, grad_new, H_new = full(u_new)
        gnorm_new = float(np.linalg.norm(grad_new))
        n_iter += 1
        if f_new >= f and gnorm_new >= gnorm:   # a step inside the slack that did not help: u is the float64 optimum
            break
        u, f, grad, H, gnorm = u_new, f_new, grad_new, H_new, gnorm_new
        converged = gnorm <= tol * gnorm0
    if not converged and n_iter >= max_iter:
        warnings.warn(f"newton_fit: {max_iter} Newton iterations ended at |g| / |g(0)| = {gnorm / gnorm0:.3e} > {tol:.3e}", RuntimeWarning,
                      stacklevel=2)
    w, b = split(u)
    return NewtonResult(w=w.copy(), b=b, n_iter=n_iter, n_evals=n_evals, converged=bool(converged), grad_norm=gnorm, grad_norm0=gnorm0)


def _cholesky_solve(H: np.ndarray, rhs: np.ndarray) -> np.ndarray:
    """H p = rhs for a symmetric positive definite H (LAPACK potrf / potrs through torch); a ridge, grown tenfold, where the
    unpenalised intercept leaves H singular to rounding"""
    Ht = torch.from_numpy(np.ascontiguousarray(H))
    ridge = 0.0
    for _ in range(20):
        L, info = torch.linalg.cholesky_ex(Ht if ridge == 0.0 else Ht + ridge * torch.eye(len(H), dtype=torch.float64))
        if int(info) == 0:
            return torch.cholesky_solve(torch.from_numpy(np.ascontiguousarray(rhs))[:, None], L)[:, 0].numpy()
        ridge = max(10.0 * ridge, 1e-12 * float(np.abs(np.diag(H)).max()))
    raise np.linalg.LinAlgError("the Newton system is not positive definite")


# ------------------------------------------------------------------------------------------------ sklearn's rules, restated
def class_weights(class_weight, classes: np.ndarray, y_idx: np.ndarray) -> np.ndarray:
    """``sklearn.utils.class_weight.compute_class_weight``: None -> ones; "balanced" -> n / (K bincount); a dict -> its values, 1
    for a class it does not name (an error where it names a class that is not there)"""
    K = len(classes)
    if class_weight is None:
        return np.ones(K)
    if isinstance(class_weight, str):
        if class_weight != "balanced":
            raise ValueError(f"class_weight={class_weight!r} must be None, 'balanced' or a dict")
        return len(y_idx) / (K * np.bincount(y_idx, minlength=K).astype(np.float64))
    if not isinstance(class_weight, dict):
        raise ValueError(f"class_weight={class_weight!r} must be None, 'balanced' or a dict")
    known = list(classes.tolist())
    missing = [c for c in class_weight if c not in known]
    if missing:
        raise ValueError(f"The classes, {missing}, are not in class_weight's data")
    return np.array([float(class_weight.get(c, 1.0)) for c in known])


def stratified_split(y, train_size: float, seed: int) -> tuple[np.ndarray, np.ndarray]:
    """-> (train, test) row indices of ``train_test_split(..., train_size=train_size, random_state=seed, stratify=y,
    shuffle=True)``, in sklearn's order: ``n_train = floor(train_size n)``, the rest is the test part; class allocations by
    ``approximate_mode`` and one permutation per class (``evalkit.stratified_shuffle_parts``), then one of each part."""
    y = np.asarray(y)
    n = len(y)
    n_train = int(np.floor(train_size * n))
    n_test = n - n_train
    classes, counts = np.unique(y, return_counts=True)
    if n_train < 1 or n_test < 1:
        raise ValueError(f"train_size={train_size} leaves an empty part of {n} rows")
    if counts.min() < 2:
        raise ValueError("The least populated class in y has only 1 member, which is too few.")
    if n_train < len(classes) or n_test < len(classes):
        raise ValueError(f"train ({n_train}) and test ({n_test}) parts must each hold at least one row per class ({len(classes)})")
    rng = np.random.RandomState(seed)
    train, test = stratified_shuffle_parts(y, n_train, n_test, rng)
    return rng.permutation(train), rng.permutation(test)


def group_shuffle_split(groups, train_size: float, seed: int) -> tuple[np.ndarray, np.ndarray]:
    """-> (train, test) row indices, ascending, of ``GroupShuffleSplit(n_splits=1, train_size=train_size,
    random_state=seed)``: one permutation of the distinct groups, the first ``n_groups - floor(train_size n_groups)`` of it are
    the test groups, the rest the train groups"""
    uniq, gidx = np.unique(np.asarray(groups), return_inverse=True)
    gidx = gidx.reshape(-1)
    ng = len(uniq)
    n_train = int(np.floor(train_size * ng))
    n_test = ng - n_train
    if n_train < 1 or n_test < 1:
        raise ValueError(f"train_size={train_size} leaves an empty part of {ng} groups")
    perm = np.random.RandomState(seed).permutation(ng)
    test_g, train_g = perm[:n_test], perm[n_test: n_test + n_train]
    return np.flatnonzero(np.isin(gidx, train_g)), np.flatnonzero(np.isin(gidx, test_g))


def classification_report(y_true, y_pred) -> dict:
    """the numbers of ``sklearn.metrics.classification_report(output_dict=True)``: per label of ``unique(y_true | y_pred)``
    (keyed by ``str``) precision, recall, f1-score and support, ``accuracy``, and the ``macro avg`` / ``weighted avg`` rows; a 0 / 0
    is 0"""
    y_true, y_pred = np.asarray(y_true), np.asarray(y_pred)
    labels = np.unique(np.concatenate((y_true, y_pred)))
    rows = {}
    P, R, F, N = [], [], [], []
    for c in labels:
        tp = float(np.sum((y_true == c) & (y_pred == c)))
        n_pred, n_true = float(np.sum(y_pred == c)), float(np.sum(y_true == c))
        p = tp / n_pred if n_pred else 0.0
        r = tp / n_true if n_true else 0.0
        f = 2.0 * p * r / (p + r) if p + r else 0.0
        rows[str(c)] = {"precision": p, "recall": r, "f1-score": f, "support": n_true}
        P.append(p), R.append(r), F.append(f), N.append(n_true)
    P, R, F, N = (np.array(v) for v in (P, R, F, N))
    rows["accuracy"] = float(np.mean(y_true == y_pred))
    rows["macro avg"] = {"precision": float(P.mean()), "recall": float(R.mean()), "f1-score": float(F.mean()), "support": float(N.sum())}
    rows["weighted avg"] = {"precision": float(np.average(P, weights=N)), "recall": float(np.average(R, weights=N)),
                            "f1-score": float(np.average(F, weights=N)), "support": float(N.sum())}
    return rows


def roc_auc(positive, score) -> float:
    """the area under the ROC curve by tie-averaged ranks (Mann-Whitney): ``positive`` a boolean vector; ``ValueError`` where
    only one class is present, as ``sklearn.metrics.roc_auc_score``"""
    positive = np.asarray(positive, dtype=bool)
    n_pos = int(positive.sum())
    n_neg = len(positive) - n_pos
    if n_pos == 0 or n_neg == 0:
        raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
    ranks = average_ranks(np.asarray(score, dtype=np.float64))
    return float((ranks[positive].sum() - n_pos * (n_pos + 1) / 2.0) / (float(n_pos) * float(n_neg)))


def _auroc(y_true, proba, classes) -> float:
    """the reference's choice: the positive column for two classes, else one-vs-rest macro (``ValueError`` unless every class is
    present, as sklearn's)"""
    y_true = np.asarray(y_true)
    if len(classes) == 2:
        return roc_auc(y_true == classes[1], proba[:, 1])
    present = np.unique(y_true)
    if len(present) != len(classes):
        raise ValueError("Number of classes in y_true not equal to the number of columns in 'y_score'")
    return float(np.mean([roc_auc(y_true == c, proba[:, i]) for i, c in enumerate(classes)]))


# ------------------------------------------------------------------------------------------------ the estimator
class _DeviceObjective:
    """``evaluate`` of ``newton_fit`` on the device: the row pass, the weighted column sums and the row-scaled Gram"""

    def __init__(self, x: Tensor, labels: Tensor, pos: int, cp: float, cn: float):
        self.x, self.labels, self.pos, self.cp, self.cn = x, labels, int(pos), float(cp), float(cn)

    def __call__(self, w, b, want_hessian):
        from . import ops

        wd = upload(w, self.x.device, np.float64)
        out = ops.logreg_rows(self.x, wd, float(b), self.labels, self.pos, self.cp, self.cn, derivatives=bool(want_hessian))
        if not want_hessian:
            return float(out["sums"][0]), None, None, None, None, None
        gh = ops.wcolsum(self.x, out["rs"])
        G = ops.gram_scaled(self.x, out["q"])
        sums, gh = out["sums"].cpu().numpy(), gh.cpu().numpy()
        return float(sums[0]), gh[0], float(sums[1]), G.cpu().numpy(), gh[1], float(sums[2])


class LogisticRegression:
    """``sklearn.linear_model.LogisticRegression`` for the objectives of the module docstring: ``classes_``, ``coef_``
    ((1, d) for two classes, else (K, d)), ``intercept_``, ``n_iter_`` (Newton iterations per problem), ``n_features_in_``, float64.
    Inputs are numpy arrays or torch tensors; a tensor already on the device is used in place.  ``fit_info_`` keeps the
    ``NewtonResult`` of every problem."""

    def __init__(self, penalty="l2", *, dual=False, tol=1e-4, C=1.0, fit_intercept=True, intercept_scaling=1, class_weight=None,
                 random_state=None, solver="lbfgs", max_iter=100, multi_class="deprecated", verbose=0, warm_start=False, n_jobs=None,
                 l1_ratio=None):
        self.penalty, self.dual, self.tol, self.C = penalty, dual, tol, C
        self.fit_intercept, self.intercept_scaling, self.class_weight = fit_intercept, intercept_scaling, class_weight
        self.random_state, self.solver, self.max_iter, self.multi_class = random_state, solver, max_iter, multi_class
        self.verbose, self.warm_start, self.n_jobs, self.l1_ratio = verbose, warm_start, n_jobs, l1_ratio

    def _check_served(self, n_classes: int, sample_weight) -> None:
        if self.solver not in SOLVERS:
            raise ValueError(f"solver={self.solver!r} must be one of {SOLVERS}")
        if sample_weight is not None:
            raise NotImplementedError("sample_weight is not built (class_weight is)")
        if self.penalty != "l2":
            raise NotImplementedError(f"penalty={self.penalty!r} is not built (the Newton solver serves 'l2')")
        if self.l1_ratio is not None:
            raise NotImplementedError(f"l1_ratio={self.l1_ratio!r} is not built (the Newton solver serves penalty='l2')")
        if self.dual:
            raise NotImplementedError("dual=True is not built (the primal objective is)")
        if self.multi_class not in ("deprecated", "auto", "ovr"):
            raise NotImplementedError(f"multi_class={self.multi_class!r} is not built")
        if self.warm_start:
            raise NotImplementedError("warm_start=True is not built")
        if n_classes > 2 and self.solver != "liblinear":
            raise NotImplementedError(f"multinomial logistic regression ({n_classes} classes with solver={self.solver!r}) is not built: "
                                      "solver='liblinear' fits one-vs-rest")
        if not float(self.C) > 0.0:
            raise ValueError(f"C={self.C!r} must be positive")

    def problems(self, classes: np.ndarray, y_idx: np.ndarray) -> list[tuple[int, float, float]]:
        """-> [(positive class index, cp, cn)]: one problem for two classes, else one per class (the module docstring's rule)"""
        wt = class_weights(self.class_weight, classes, y_idx)
        C = float(self.C)
        if len(classes) == 2:
            return [(1, C * wt[1], C * wt[0])]
        return [(k, C * wt[k], C) for k in range(len(classes))]

    def tolerance(self, n_pos: int, n: int) -> float:
        return min(float(self.tol) * max(min(n_pos, n - n_pos), 1) / n, 1e-10)

    def fit(self, X, y, sample_weight=None):
        X = as_matrix(X, min_rows=2, min_cols=1)
        y = np.asarray(y)
        if y.ndim != 1 or len(y) != X.shape[0]:
            raise ValueError(f"y {y.shape} must hold one label per row of X {tuple(X.shape)}")
        classes, y_idx = np.unique(y, return_inverse=True)
        y_idx = y_idx.reshape(-1)
        if len(classes) < 2:
            raise ValueError(f"This solver needs samples of at least 2 classes in the data, but the data contains only one class: {classes[0]!r}")
        self._check_served(len(classes), sample_weight)
        served(X.shape[1])
        x = to_device(X, device_of(X, who="reduce"))
        n, d = x.shape
        labels = upload(y_idx, x.device, np.int32)
        liblinear = self.solver == "liblinear"
        results = []
        for pos, cp, cn in self.problems(classes, y_idx):
            res = newton_fit(_DeviceObjective(x, labels, pos, cp, cn), d, penalised_intercept=liblinear,
                             intercept_scaling=float(self.intercept_scaling), tol=self.tolerance(int((y_idx == pos).sum()), n),
                             max_iter=int(self.max_iter), fit_intercept=bool(self.fit_intercept))
            results.append(res)
        self.classes_ = classes
        self.coef_ = np.stack([r.w for r in results])
        self.intercept_ = np.array([r.b for r in results])
        self.n_iter_ = np.array([r.n_iter for r in results], dtype=np.int32)
        self.n_features_in_ = int(d)
        self.fit_info_ = results
        return self

    def _margins(self, X) -> np.ndarray:
        from . import ops

        if not hasattr(self, "coef_"):
            raise RuntimeError("this LogisticRegression is not fitted yet")
        X = as_matrix(X, width=self.n_features_in_, finite=False)
        x = to_device(X, device_of(X, who="reduce"))
        if x.shape[0] == 0:
            return np.zeros((0, len(self.coef_)))
        x, n = padded_to_two_rows(x)
        z = [ops.logreg_margins(x, upload(w, x.device), float(b)) for w, b in zip(self.coef_, self.intercept_)]
        return torch.stack(z, dim=1).cpu().numpy()[:n]

    def decision_function(self, X) -> np.ndarray:
        z = self._margins(X)
        return z[:, 0] if z.shape[1] == 1 else z

    def predict(self, X) -> np.ndarray:
        z = self._margins(X)
        idx = (z[:, 0] > 0).astype(np.int64) if z.shape[1] == 1 else np.argmax(z, axis=1)
        return self.classes_[idx]

    def predict_proba(self, X) -> np.ndarray:
        z = self._margins(X)
        e = np.exp(-np.abs(z))
        big, small = 1.0 / (1.0 + e), e / (1.0 + e)   # sigma and 1 - sigma without cancellation
        sig = np.where(z >= 0, big, small)
        if z.shape[1] == 1:
            return np.concatenate((np.where(z >= 0, small, big), sig), axis=1)
        return sig / sig.sum(axis=1, keepdims=True)

    def predict_log_proba(self, X) -> np.ndarray:
        return np.log(self.predict_proba(X))

    def score(self, X, y) -> float:
        return float(np.mean(self.predict(X) == np.asarray(y)))


# ------------------------------------------------------------------------------------------------ the reference module's surface
def _scale_on_device(scaler: StandardScaler, x: Tensor) -> Tensor:
    return project(x, scaler.mean_, scaler.projection_weights())


def _reduce_on_device(pca: PCA, x: Tensor) -> Tensor:
    return project(x, pca.fit_.data_mean, pca.fit_.projection_weights())


class LinearClassifierPipeline:
    """a fitted classifier with its preprocessing (``scaler`` and ``pca`` may be None), the training ``config`` and the ``task``"""

    def __init__(self, classifier: LogisticRegression, scaler: StandardScaler | None, pca: PCA | None, config: dict, task: str):
        self.classifier, self.scaler, self.pca, self.config, self.task = classifier, scaler, pca, config, task

    def _transform(self, X) -> Tensor:
        """the preprocessing on the device: X goes there once and stays"""
        X = as_matrix(X, finite=False)
        x, n = padded_to_two_rows(to_device(X, device_of(X, who="reduce")))
        if self.scaler is not None:
            x = _scale_on_device(self.scaler, x)
        if self.pca is not None:
            x = _reduce_on_device(self.pca, x)
        return x[:n]

    def transform(self, X) -> np.ndarray:
        return self._transform(X).cpu().numpy()

    def predict(self, X) -> np.ndarray:
        return self.classifier.predict(self._transform(X))

    def predict_proba(self, X) -> np.ndarray:
        return self.classifier.predict_proba(self._transform(X))


def _metrics(prefix: str, y, pred, proba, classes) -> dict:
    rep = classification_report(y, pred)
    out = {f"{prefix}_accuracy": rep["accuracy"]}
    for key in ("precision", "recall", "f1"):
        out[f"{prefix}_weighted_{key}"] = rep["weighted avg"]["f1-score" if key == "f1" else key]
    try:
        out[f"{prefix}_auroc"] = _auroc(y, proba, classes)
        if prefix == "val" and len(classes) > 2:
            for i, c in enumerate(classes):
                try:
                    out[f"val_{c}_auroc"] = roc_auc(np.asarray(y) == c, proba[:, i])
                except ValueError:
                    pass
    except ValueError as e:
        _logger.warning(f"Could not compute {prefix} AUROC (likely only one class present): {e}")
    for c in classes:
        if str(c) in rep:
            row = rep[str(c)]
            out[f"{prefix}_{c}_precision"], out[f"{prefix}_{c}_recall"] = row["precision"], row["recall"]
            out[f"{prefix}_{c}_f1"], out[f"{prefix}_{c}_support"] = row["f1-score"], int(row["support"])
    return out


def train_linear_classifier(adata, task: str, use_scaling: bool = True, use_pca: bool = False, n_pca_components: int | None = None,
                            classifier_params: dict[str, Any] | None = None, split_train_data: float = 0.8, random_seed: int = 42,
                            groups=None) -> tuple[LinearClassifierPipeline, dict[str, float], dict[str, Any]]:
    """-> (pipeline, metrics, val_outputs) as the reference: ``adata.X`` are the embeddings, ``adata.obs[task]`` the labels.
    ``StandardScaler`` and ``PCA(n_pca_components)`` are fitted on all rows; the train / validation split is
    ``train_test_split(stratify=y)``, or ``GroupShuffleSplit`` over ``groups`` (no group in both parts); ``split_train_data=1.0``
    trains on everything and returns no validation keys.  Metrics: ``{train,val}_accuracy``, ``_weighted_{precision,recall,f1}``,
    ``_auroc``, per class ``_{class}_{precision,recall,f1,support}`` and, for more than two classes, ``val_{class}_auroc``.
    ``val_outputs``: ``y_val``, ``y_val_proba`` (rows in the split's order), ``classes``.  The embeddings go to the device once."""
    classifier_params = {} if classifier_params is None else classifier_params
    X_full = adata.X if isinstance(adata.X, np.ndarray) or torch.is_tensor(adata.X) else adata.X.toarray()
    y_full = adata.obs[task].to_numpy(dtype=object)
    X_full = as_matrix(X_full, min_rows=2, min_cols=1)
    x = to_device(X_full, device_of(X_full, who="reduce"))
    scaler = pca = None
    if use_scaling:
        scaler = StandardScaler().fit(x)
        x = _scale_on_device(scaler, x)
    if use_pca:
        pca = PCA(n_components=n_pca_components).fit(x)
        x = _reduce_on_device(pca, x)

    idx_val = None
    if split_train_data < 1.0:
        if groups is not None:
            if len(groups) != len(y_full):
                raise ValueError(f"groups length {len(groups)} != n_cells {len(y_full)}")
            idx_train, idx_val = group_shuffle_split(groups, split_train_data, random_seed)
        else:
            idx_train, idx_val = stratified_split(y_full, split_train_data, random_seed)
        x_train, y_train = x[torch.from_numpy(idx_train).to(x.device)], y_full[idx_train]
        x_val, y_val = x[torch.from_numpy(idx_val).to(x.device)], y_full[idx_val]
    else:
        x_train, y_train, x_val, y_val = x, y_full, None, None

    classifier = LogisticRegression(**classifier_params).fit(x_train, y_train)
    classes = classifier.classes_
    metrics = _metrics("train", y_train, classifier.predict(x_train), classifier.predict_proba(x_train), classes)
    y_val_proba = None
    if x_val is not None:
        y_val_proba = classifier.predict_proba(x_val)
        metrics.update(_metrics("val", y_val, classifier.predict(x_val), y_val_proba, classes))

    config = {"task": task, "use_scaling": use_scaling, "use_pca": use_pca, "n_pca_components": n_pca_components,
              "classifier_params": classifier_params, "split_train_data": split_train_data, "random_seed": random_seed}
    pipeline = LinearClassifierPipeline(classifier=classifier, scaler=scaler, pca=pca, config=config, task=task)
    return pipeline, metrics, {"y_val": y_val, "y_val_proba": y_val_proba, "classes": classes.tolist()}


def predict_with_classifier(adata, pipeline: LinearClassifierPipeline, task: str, artifact_metadata: dict | None = None,
                            include_wells: list[str] | None = None):
    """Writes ``adata.obs["predicted_{task}"]``, ``adata.obsm["predicted_{task}_proba"]`` and
    ``adata.uns["predicted_{task}_classes"]`` and returns ``adata``.  ``include_wells`` (prefixes such as ``"A/1"`` of
    ``obs["fov_name"]``) restricts the prediction: the other rows hold NaN.  ``artifact_metadata`` (``artifact_name``,
    ``artifact_id``, ``artifact_version``) is recorded under ``classifier_{task}_artifact`` / ``_id`` / ``_version``."""
    n = len(adata.obs)
    if include_wells is not None:
        mask = adata.obs["fov_name"].str.startswith(tuple(w + "/" for w in include_wells)).to_numpy(dtype=bool)
    else:
        mask = np.ones(n, dtype=bool)
    X_full = adata.X if isinstance(adata.X, np.ndarray) or torch.is_tensor(adata.X) else adata.X.toarray()
    classes = pipeline.classifier.classes_
    predictions = np.full(n, np.nan, dtype=object)
    proba = np.full((n, len(classes)), np.nan)
    if mask.any():
        rows = np.flatnonzero(mask)
        X_subset = X_full[torch.from_numpy(rows).to(X_full.device)] if torch.is_tensor(X_full) else X_full[rows]
        x = pipeline._transform(X_subset)
        predictions[mask] = pipeline.classifier.predict(x)
        proba[mask] = pipeline.classifier.predict_proba(x)
    adata.obs[f"predicted_{task}"] = predictions
    adata.obsm[f"predicted_{task}_proba"] = proba
    adata.uns[f"predicted_{task}_classes"] = classes.tolist()
    if artifact_metadata is not None:
        adata.uns[f"classifier_{task}_artifact"] = artifact_metadata["artifact_name"]
        adata.uns[f"classifier_{task}_id"] = artifact_metadata["artifact_id"]
        adata.uns[f"classifier_{task}_version"] = artifact_metadata["artifact_version"]
    return adata
