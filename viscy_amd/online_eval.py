"""``viscy_utils.callbacks.OnlineEvalCallback`` (callbacks/online_eval.py) with the embeddings left on the device: every
``every_n_epochs`` validation epochs it logs

* ``metrics/knn_acc/<label_key>/val`` — cosine k-NN accuracy under stratified 5-fold cross-validation or a stratified holdout
* ``metrics/effective_rank/val``      — exp of the entropy of the normalised singular values
* ``metrics/temporal_smoothness/val`` — Spearman rho of |dt| against cosine distance over all pairs inside a track

The reference computes the three on the host (sklearn's brute-force k-NN once per fold, a numpy SVD, a Python loop over the pairs).
Here the k-NN probe is one pass of ``vsx_knn_topk`` for all folds at once: a fold is a *group*, and a row's candidates are the
rows of the other groups, which is exactly "fit on the other folds, predict this one"; the N x N similarity matrix is never
stored.  The splits themselves are O(N) host work and restate sklearn's draw for draw (``stratified_kfold_ids``,
``stratified_holdout_ids``), so the folds are the reference's folds.  The holdout's draw and the tie-averaged ranks are ``evalkit``'s
(``stratified_shuffle_parts``, ``average_ranks``), shared with ``linear_classifier``.

Differences from the reference, all at its edges:

* a fold (or holdout train part) with fewer than ``k`` rows votes among the rows there are (``cnt`` of them); sklearn raises there;
* neighbours with exactly equal similarity are ordered by row index (the kernel's total order); sklearn's order among exact ties
  is an artefact of its partial sort;
* ``k`` (after ``min(k, n - 1)``) above 64 is refused by the kernel;
* labels that are not integers (strings) are encoded by sorted unique value before the reference's ``np.bincount`` decision,
  where the reference raises a ``TypeError``.
"""

from __future__ import annotations

import logging
import math
import warnings
from typing import Any, Literal, Sequence

import numpy as np
import torch
import torch.distributed as dist
from torch import Tensor

from .evalkit import as_matrix, average_ranks, stratified_shuffle_parts, to_device, upload

_logger = logging.getLogger("viscy_amd")


# ------------------------------------------------------------------------------------------------ host helpers (numpy, O(N))
def stratified_kfold_ids(labels, n_splits: int) -> np.ndarray:
    """the test fold of every row under sklearn's ``StratifiedKFold(n_splits, shuffle=False)``: classes encoded by first
    appearance, ``allocation[i] = bincount(sort(y_enc)[i::n_splits])``, and per class the folds ``arange(n_splits)`` repeated by
    its allocation, handed out in row order"""
    y = np.asarray(labels)
    _, first, inv = np.unique(y, return_index=True, return_inverse=True)
    _, class_perm = np.unique(first, return_inverse=True)
    y_enc = class_perm[inv.reshape(-1)]
    n_classes = len(first)
    counts = np.bincount(y_enc)
    if n_splits < 2 or n_splits > counts.max():
        raise ValueError(f"n_splits={n_splits} must be in [2, {counts.max()}] (the largest class)")
    y_order = np.sort(y_enc)
    allocation = np.asarray([np.bincount(y_order[i::n_splits], minlength=n_classes) for i in range(n_splits)])
    folds = np.empty(len(y_enc), dtype=np.int64)
    for c in range(n_classes):
        folds[y_enc == c] = np.arange(n_splits).repeat(allocation[:, c])
    return folds


def stratified_holdout_ids(labels, test_size: float, seed: int = 0) -> np.ndarray:
    """1 for the rows ``train_test_split(..., test_size=test_size, stratify=labels, random_state=seed)`` puts into the test part,
    0 for its train part.  That split is one draw of ``StratifiedShuffleSplit``: ``n_test = ceil(test_size * n)``, class
    allocations and one permutation per class by ``evalkit.stratified_shuffle_parts``."""
    y = np.asarray(labels)
    n = len(y)
    n_test = int(math.ceil(test_size * n))
    n_train = n - n_test
    counts = np.unique(y, return_counts=True)[1]
    n_classes = len(counts)
    if counts.min() < 2:
        raise ValueError("The least populated class has only 1 member: a stratified holdout needs 2 per class")
    if n_train < n_classes or n_test < n_classes:
        raise ValueError(f"train ({n_train}) and test ({n_test}) parts must each hold at least one row per class ({n_classes})")
    train, test = stratified_shuffle_parts(y, n_train, n_test, np.random.RandomState(seed))
    ids = np.full(n, -1, dtype=np.int64)
    ids[train], ids[test] = 0, 1
    assert (ids >= 0).all()  # n_train + n_test = n: every row lands in one part
    return ids


def track_pairs(track_ids, min_track_len: int = 2) -> tuple[np.ndarray, np.ndarray]:
    """all row pairs ``i < j`` inside each track: tracks in ``np.unique`` order, rows of a track in row order, pairs
    (0,1), (0,2), ..., (1,2), ... — the order of the reference's loops; vectorised (one block per distinct track length)"""
    tid = np.asarray(track_ids)
    order = np.argsort(tid, kind="stable")
    _, starts, sizes = np.unique(tid[order], return_index=True, return_counts=True)
    npairs = np.where(sizes >= min_track_len, sizes * (sizes - 1) // 2, 0)
    offs = np.concatenate(([0], np.cumsum(npairs)))
    pi = np.empty(offs[-1], dtype=np.int64)
    pj = np.empty(offs[-1], dtype=np.int64)
    for n in np.unique(sizes[npairs > 0]):
        a, b = np.triu_indices(int(n), 1)
        sel = np.nonzero((sizes == n) & (npairs > 0))[0]
        out = (offs[sel][:, None] + np.arange(len(a))[None, :]).reshape(-1)
        pi[out] = order[(starts[sel][:, None] + a[None, :]).reshape(-1)]
        pj[out] = order[(starts[sel][:, None] + b[None, :]).reshape(-1)]
    return pi, pj


def spearman_rho(a, b) -> float:
    """Spearman's rho: the Pearson correlation of the two tie-averaged rank vectors, in float64 (NaN for a constant vector)"""
    ra, rb = average_ranks(a), average_ranks(b)
    if torch.is_tensor(ra) or torch.is_tensor(rb):
        dev = ra.device if torch.is_tensor(ra) else rb.device
        ra, rb = (r if torch.is_tensor(r) else torch.from_numpy(r).to(dev) for r in (ra, rb))
        ra, rb = ra - ra.mean(), rb - rb.mean()
        return float(((ra * rb).sum() / torch.sqrt((ra * ra).sum() * (rb * rb).sum())).item())
    ra, rb = ra - ra.mean(), rb - rb.mean()
    with np.errstate(invalid="ignore", divide="ignore"):
        return float((ra * rb).sum() / np.sqrt((ra * ra).sum() * (rb * rb).sum()))


# ------------------------------------------------------------------------------------------------ device functions
def knn_predict(features: Tensor, labels, group, k: int) -> tuple[Tensor, Tensor, np.ndarray]:
    """-> (pred, y, classes): for every row the vote (index into ``classes``, int32 on the device; -1 without candidates) of its
    ``k`` cosine-nearest rows among the other groups (``group >= 0`` and different from the row's), and the encoded labels"""
    from . import ops

    features = as_matrix(features)  # non-finite values: sklearn's check_array message
    classes, y = np.unique(np.asarray(labels), return_inverse=True)
    x = to_device(features, features.device)
    y_d = upload(y.reshape(-1), x.device, np.int32)
    g_d = upload(np.asarray(group).reshape(-1), x.device, np.int32)
    inv = ops.row_inv_norm(x, 0.0)
    idx, _, cnt = ops.knn_topk(x, inv, g_d, k)
    return ops.knn_vote(idx, cnt, y_d), y_d, classes


def knn_accuracy(features: Tensor, labels, group, k: int, score_groups: Sequence[int]) -> float:
    """the mean over ``score_groups`` of the accuracy of ``knn_predict`` on the rows of that group.  Cross-validation: ``group`` =
    the fold ids and every fold is scored (``cross_val_score(...).mean()``); holdout: ``group`` = 0 (train) / 1 (test) and only
    group 1 is scored.  A group with fewer than ``k`` candidate rows votes among those there are."""
    pred, y, _ = knn_predict(features, labels, group, k)
    g_d = upload(np.asarray(group).reshape(-1), pred.device, np.int64)
    hit = (pred == y).to(torch.float64)
    accs = torch.stack([hit[g_d == int(g)].mean() for g in score_groups])
    return float(accs.mean().item())


def _rank_zero() -> bool:
    return not dist.is_initialized() or dist.get_rank() == 0


def effective_rank(features: Tensor) -> float:
    """exp of the Shannon entropy of the normalised singular values (Roy & Bhattacharya 2007), as the reference's
    ``effective_rank``: rows with a non-finite entry are dropped (one warning, on rank 0), fewer than 2 rows give NaN, singular
    values <= 1e-10 are left out.  The singular values are those of the feature matrix itself, not of its Gram matrix (which
    would square the condition number): a float64 Householder QR on the tensor's device reduces the (N, d) matrix to its
    triangular factor (O(N d^2), the part that grows with the validation set), and the singular values of that d x d factor
    come from LAPACK on the host.  The device SVD behind ``torch.linalg.svdvals`` returned float64 singular values with an
    absolute error of about 1e-7 of the largest one on the MI355X stack this was measured on, whatever the driver; on
    embeddings of low rank, whose many tiny singular values all enter the entropy, that is more than the reference's own
    fp32-against-float64 difference."""
    x = features.detach()
    finite = torch.isfinite(x).all(dim=1)
    n_bad = int((~finite).sum())
    if n_bad:
        if _rank_zero():
            warnings.warn(f"effective_rank: {n_bad}/{x.shape[0]} rows contain NaN/Inf; skipping those")
        x = x[finite]
    if x.shape[0] < 2:
        return float("nan")
    r = torch.linalg.qr(x.to(torch.float64), mode="r").R
    s = torch.linalg.svdvals(r.cpu())
    s = s[s > 1e-10]
    if s.numel() == 0:
        return float("nan")
    p = s / s.sum()
    return float(torch.exp(-(p * torch.log(p)).sum()).item())


def temporal_smoothness(features: Tensor, track_ids, timepoints) -> float:
    """Spearman rho between |t_i - t_j| and the cosine distance 1 - cos(x_i, x_j) (rows normalised by ``||x|| + 1e-10``, as the
    reference) over all pairs inside a track; NaN with fewer than 3 pairs"""
    from . import ops

    pi, pj = track_pairs(track_ids)
    if len(pi) < 3:
        return float("nan")
    x = to_device(features.detach(), features.device)
    t = np.asarray(timepoints).reshape(-1).astype(np.float64)
    dt = np.abs(t[pi] - t[pj])
    inv = ops.row_inv_norm(x, 1e-10)
    dev = x.device
    dist_ = ops.pair_cosine_dist(x, inv, upload(pi, dev, np.int32), upload(pj, dev, np.int32))
    return spearman_rho(upload(dt, dev), dist_)


# ------------------------------------------------------------------------------------------------ the callback
class OnlineEvalCallback:
    """Drop-in for ``viscy_utils.callbacks.OnlineEvalCallback``: same keywords and defaults, same hooks
    (``on_validation_epoch_start`` / ``on_validation_batch_end`` / ``on_validation_epoch_end``), same decisions.  Embeddings are
    collected on the device (no ``.cpu()``); metrics are logged through the module's ``_log(key, value)``.

    Decisions mirrored from the reference: ``k = min(k, n - 1)``; the k-NN probe runs only with labels present and at least two
    unique values; ``min_class_count = min(np.bincount(labels))`` — so integer labels with a gap (say 0 and 2) count 0 for the
    missing value and skip the probe; ``"cv"`` degrades to ``"holdout"`` when the smallest class has fewer than 2 rows;
    ``cv_folds = min(5, min_class_count)``; holdout needs at least 2 rows per class; the smoothness is logged only when it is
    not NaN.  Under ``torch.distributed`` every rank truncates to the smallest row count, all-gathers features and numeric
    metadata (strings through ``all_gather_object``) and computes on the full set; a key that any rank lacks is missing for all.

    A fold whose training part has fewer than ``k`` rows votes among the rows available (sklearn would raise there).
    Non-finite features raise ``ValueError`` in the k-NN probe, as sklearn does."""

    def __init__(self, every_n_epochs: int = 5, label_key: str = "marker", k: int = 20, track_id_key: str = "global_track_id",
                 timepoint_key: str = "t", knn_eval_mode: Literal["cv", "holdout"] = "cv", holdout_test_size: float = 0.2):
        self.every_n_epochs = every_n_epochs
        self.label_key = label_key
        self.k = k
        self.track_id_key = track_id_key
        self.timepoint_key = timepoint_key
        self.knn_eval_mode = knn_eval_mode
        self.holdout_test_size = holdout_test_size
        self._collecting = False
        self._features: list[Tensor] = []
        self._meta: list[dict] = []

    def _should_collect(self, trainer) -> bool:
        return trainer.current_epoch % self.every_n_epochs == 0 and not trainer.sanity_checking

    def _reset(self) -> None:
        self._collecting = False
        self._features = []
        self._meta = []

    def on_validation_epoch_start(self, trainer, pl_module) -> None:
        if self._should_collect(trainer):
            self._collecting = True

    def on_validation_batch_end(self, trainer, pl_module, outputs: Any, batch, batch_idx: int, dataloader_idx: int = 0) -> None:
        if not self._collecting:
            return
        with torch.no_grad():
            features, _ = pl_module(batch["anchor"])
        self._features.append(features.detach())
        self._meta.extend(batch.get("anchor_meta", []))

    def on_validation_epoch_end(self, trainer, pl_module) -> None:
        if not self._collecting or not self._features:
            self._reset()
            return
        features_local = torch.cat(self._features).float()
        features, labels, track_ids, timepoints = self._gather_across_ranks(
            features_local, self._extract_array(self.label_key, source="labels"),
            self._extract_array(self.track_id_key, source="meta"), self._extract_array(self.timepoint_key, source="meta"))
        n_samples = features.shape[0]
        epoch = trainer.current_epoch
        is_rank_zero = getattr(trainer, "global_rank", 0) == 0

        erank = effective_rank(features)
        pl_module._log("metrics/effective_rank/val", erank)
        if is_rank_zero:
            _logger.info(f"[OnlineEval epoch {epoch}] effective_rank={erank:.1f} (n={n_samples}, d={features.shape[1]})")

        if labels is not None and len(np.unique(labels)) >= 2:
            k = min(self.k, n_samples - 1)
            if labels.dtype.kind not in "iub":  # the reference's np.bincount raises on these
                labels = np.unique(labels, return_inverse=True)[1].reshape(-1)
            min_class_count = int(min(np.bincount(labels)))
            mode = self.knn_eval_mode
            if mode == "cv" and min_class_count < 2:
                mode = "holdout"
            knn_acc = None
            if mode == "cv":
                cv_folds = min(5, min_class_count)
                knn_acc = knn_accuracy(features, labels, stratified_kfold_ids(labels, cv_folds), k, range(cv_folds))
                eval_desc = f"cv={cv_folds}"
            elif mode == "holdout" and min_class_count >= 2:
                knn_acc = knn_accuracy(features, labels, stratified_holdout_ids(labels, self.holdout_test_size, seed=0), k, (1,))
                eval_desc = f"holdout={self.holdout_test_size:.2f}"
            elif is_rank_zero:
                _logger.debug(f"[OnlineEval epoch {epoch}] Skipping k-NN: smallest class has {min_class_count} samples (need >=2).")
            if knn_acc is not None:
                pl_module._log(f"metrics/knn_acc/{self.label_key}/val", knn_acc)
                if is_rank_zero:
                    _logger.info(f"[OnlineEval epoch {epoch}] knn_acc({self.label_key}, k={k})={knn_acc:.3f} ({eval_desc})")

        if track_ids is not None and timepoints is not None:
            rho = temporal_smoothness(features, track_ids, timepoints)
            if not np.isnan(rho):
                pl_module._log("metrics/temporal_smoothness/val", rho)
                if is_rank_zero:
                    _logger.info(f"[OnlineEval epoch {epoch}] temporal_smoothness={rho:.3f}")
        self._reset()

    def _extract_array(self, key: str, source: Literal["labels", "meta"] = "meta") -> np.ndarray | None:
        """per-sample values of ``meta[i]["labels"][key]`` (source "labels") or ``meta[i][key]``; None if any sample lacks it"""
        values = []
        for m in self._meta:
            v = m.get("labels", {}).get(key) if source == "labels" else m.get(key)
            if v is None:
                return None
            values.append(v)
        return np.array(values)

    @staticmethod
    def _gather_across_ranks(features_local: Tensor, labels_local, track_ids_local, timepoints_local):
        """full-set (features, labels, track_ids, timepoints) on every rank; a passthrough in a single process.  Shards are
        truncated to the smallest rank's row count (``all_gather`` wants one shape); a metadata array is None for all ranks if
        any rank has none."""
        world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        if world <= 1:
            return features_local, labels_local, track_ids_local, timepoints_local
        dev = features_local.device

        def all_gather(t: Tensor) -> Tensor:
            out = [torch.empty_like(t) for _ in range(world)]
            dist.all_gather(out, t.contiguous())
            return torch.stack(out)

        n_min = int(all_gather(torch.tensor([features_local.shape[0]], device=dev)).min().item())
        features_local = features_local[:n_min]

        def gather_optional(arr):
            available = all_gather(torch.tensor([1 if arr is not None else 0], device=dev))
            if int(available.min().item()) == 0:
                return None
            arr_local = arr[:n_min]
            if arr_local.dtype.kind in {"U", "S", "O"}:
                gathered: list = [None] * world
                dist.all_gather_object(gathered, arr_local)
                return np.concatenate(gathered, axis=0)
            t = torch.as_tensor(arr_local, device=dev)
            g = all_gather(t)
            g = g.reshape(-1, *t.shape[1:]) if t.ndim > 1 else g.reshape(-1)
            return g.cpu().numpy()

        feats = all_gather(features_local)
        return (feats.reshape(-1, feats.shape[-1]), gather_optional(labels_local), gather_optional(track_ids_local),
                gather_optional(timepoints_local))
