"""CPU: the host layer under the evaluation modules (viscy_amd/evalkit.py).  The first half pins, through the public entry points of
reduce, linear_classifier, mmd and smoothness, the exception type and message of every input check, for a numpy array and for a CPU
tensor alike: it was written against the modules' own copies of these checks and passes unchanged on the shared ones.  The second half
checks the shared pieces themselves: the stratified draw against a straight restatement of sklearn's, the two-row padding, and that no
module of the package imports a private name of a sibling."""

import ast
import math
import pathlib
import types

import numpy as np
import pytest
import torch

from viscy_amd import linear_classifier as LC
from viscy_amd import mmd, reduce, smoothness
from viscy_amd import online_eval as OE

KINDS = ("numpy", "tensor")
NAN_OR_INF = r"^Input X contains NaN or infinity\.$"


def _as(kind, a):
    a = np.asarray(a, dtype=np.float32)
    return a if kind == "numpy" else torch.from_numpy(a.copy())


def _good(rows=6, d=3, seed=0):
    return np.random.RandomState(seed).randn(rows, d).astype(np.float32)


def _with(value, rows=6, d=3):
    a = _good(rows, d)
    a[2, 1] = value
    return a


@pytest.fixture(autouse=True)
def no_device(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)  # what a machine without a HIP device answers


def _fitted_scaler(d=3):
    sc = reduce.StandardScaler()
    sc.mean_, sc.var_, sc.scale_, sc.n_samples_seen_, sc.n_features_in_ = np.zeros(d), np.ones(d), np.ones(d), 6, d
    return sc


def _fitted_pca(d=3):
    pca = reduce.PCA()
    pca.fit_ = reduce.pca_from_moments(6, np.zeros(d), np.full(d, 6.0), 6.0 * np.eye(d), None, False)
    pca.n_features_in_ = d
    return pca


def _fitted_logreg(d=3):
    lr = LC.LogisticRegression()
    lr.classes_, lr.coef_, lr.intercept_, lr.n_features_in_ = np.array([0, 1]), np.ones((1, d)), np.zeros(1), d
    return lr


# ------------------------------------------------------------------------------------------------ fit: reduce._rows' rules
FITS = {
    "StandardScaler.fit": lambda X: reduce.StandardScaler().fit(X),
    "StandardScaler.fit_transform": lambda X: reduce.StandardScaler().fit_transform(X),
    "PCA.fit": lambda X: reduce.PCA().fit(X),
    "PCA.fit_transform": lambda X: reduce.PCA().fit_transform(X),
    "compute_pca": lambda X: reduce.compute_pca(X),
    "LogisticRegression.fit": lambda X: LC.LogisticRegression().fit(X, np.arange(len(X)) % 2),
}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("entry", list(FITS))
def test_fit_refusals(entry, kind):
    fit = FITS[entry]
    with pytest.raises(ValueError, match=r"^X must be a \(rows, d\) matrix, got \(3,\)$"):
        fit(_as(kind, _good()[0]))
    with pytest.raises(ValueError, match=r"^X must be a \(rows, d\) matrix, got \(2, 3, 4\)$"):
        fit(_as(kind, np.zeros((2, 3, 4))))
    with pytest.raises(ValueError, match=r"^X needs at least two rows \(got 1\)$"):
        fit(_as(kind, _good()[:1]))
    with pytest.raises(ValueError, match=r"^X needs at least two rows \(got 0\)$"):
        fit(_as(kind, _good()[:0]))
    with pytest.raises(ValueError, match=r"^X needs at least one feature$"):
        fit(_as(kind, np.zeros((4, 0))))
    with pytest.raises(ValueError, match=NAN_OR_INF):
        fit(_as(kind, _with(np.nan)))
    with pytest.raises(ValueError, match=NAN_OR_INF):
        fit(_as(kind, _with(-np.inf)))
    # the order of the checks: rows before columns before finiteness
    with pytest.raises(ValueError, match="at least two rows"):
        fit(_as(kind, np.full((1, 0), np.nan)))
    with pytest.raises(ValueError, match="at least two rows"):
        fit(_as(kind, np.full((1, 3), np.nan)))
    with pytest.raises(RuntimeError, match=r"^viscy_amd\.reduce needs the HIP device \(no CPU fallback\)$"):
        fit(_as(kind, _good()))


# ------------------------------------------------------------------------------------------------ transform: the fitted width
TRANSFORMS = {
    "StandardScaler.transform": lambda X: _fitted_scaler().transform(X),
    "PCA.transform": lambda X: _fitted_pca().transform(X),
    "LogisticRegression.decision_function": lambda X: _fitted_logreg().decision_function(X),
    "LogisticRegression.predict_proba": lambda X: _fitted_logreg().predict_proba(X),
}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("entry", list(TRANSFORMS))
def test_transform_refusals(entry, kind):
    call = TRANSFORMS[entry]
    with pytest.raises(ValueError, match=r"^X \(6, 4\) must be \(rows, 3\)$"):
        call(_as(kind, _good(6, 4)))
    with pytest.raises(ValueError, match=r"^X \(3,\) must be \(rows, 3\)$"):
        call(_as(kind, _good()[0]))
    with pytest.raises(ValueError, match=r"^X \(2, 3, 3\) must be \(rows, 3\)$"):
        call(_as(kind, np.zeros((2, 3, 3))))
    # a transform does not look at the values, and serves one row and none: the next refusal is the device's
    for X in (_with(np.nan), _with(np.inf), _good()[:1], _good()[:0], _good()):
        with pytest.raises(RuntimeError, match=r"^viscy_amd\.reduce needs the HIP device \(no CPU fallback\)$"):
            call(_as(kind, X))


def test_unfitted_estimators_say_so_before_they_look_at_x():
    for call, who in ((reduce.StandardScaler().transform, "StandardScaler"), (reduce.PCA().transform, "PCA"),
                      (LC.LogisticRegression().decision_function, "LogisticRegression")):
        with pytest.raises(RuntimeError, match=f"^this {who} is not fitted yet$"):
            call(np.zeros(3))


# ------------------------------------------------------------------------------------------------ mmd: X and Y
MMDS = {
    "compute_mmd_unbiased": lambda X, Y: mmd.compute_mmd_unbiased(X, Y, 1.0),
    "mmd_permutation_test": lambda X, Y: mmd.mmd_permutation_test(X, Y, 3, 1.0),
    "median_heuristic": lambda X, Y: mmd.median_heuristic(X, Y),
    "gaussian_rbf_kernel": lambda X, Y: mmd.gaussian_rbf_kernel(X, Y, 1.0),
}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("entry", list(MMDS))
def test_mmd_refusals(entry, kind):
    call = MMDS[entry]
    X, Y = _as(kind, _good(6, 3, 1)), _as(kind, _good(5, 3, 2))
    with pytest.raises(ValueError, match=r"^X must be a \(rows, d\) matrix, got \(3,\)$"):
        call(_as(kind, _good()[0]), Y)
    with pytest.raises(ValueError, match=r"^Y must be a \(rows, d\) matrix, got \(2, 3, 4\)$"):
        call(X, _as(kind, np.zeros((2, 3, 4))))
    with pytest.raises(ValueError, match=NAN_OR_INF):
        call(_as(kind, _with(np.nan)), Y)
    with pytest.raises(ValueError, match=NAN_OR_INF):
        call(X, _as(kind, _with(np.inf)))
    with pytest.raises(ValueError, match=r"^X \(6, 3\) and Y \(6, 4\) differ in width$"):
        call(X, _as(kind, _good(6, 4)))
    with pytest.raises(ValueError, match=NAN_OR_INF):     # the values are looked at before the widths are compared
        call(_as(kind, _with(np.nan)), _as(kind, _good(6, 4)))
    one = _as(kind, _good()[:1])
    if entry in ("compute_mmd_unbiased", "mmd_permutation_test"):
        with pytest.raises(ValueError, match=r"^the unbiased MMD\^2 needs at least two rows on either side \(got 1 and 5\)$"):
            call(one, Y)
        with pytest.raises(ValueError, match=r"^the unbiased MMD\^2 needs at least two rows on either side \(got 6 and 0\)$"):
            call(X, _as(kind, _good()[:0]))
    else:  # neither asks for two rows a side, and none asks for a column
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(one, Y)
    with pytest.raises(RuntimeError, match=r"^viscy_amd\.mmd needs the HIP device \(no CPU fallback\)$"):
        call(X, Y)
    with pytest.raises(RuntimeError, match=r"^viscy_amd\.mmd needs the HIP device \(no CPU fallback\)$"):
        call(_as(kind, np.zeros((4, 0))), _as(kind, np.zeros((4, 0))))


# ------------------------------------------------------------------------------------------------ smoothness: the device first
@pytest.mark.parametrize("kind", KINDS)
def test_smoothness_looks_for_the_device_before_it_looks_at_the_features(kind):
    obs = {"fov_name": np.array(["a"] * 6), "track_id": np.zeros(6, dtype=np.int64), "t": np.arange(6)}
    for X in (_good(), _good()[0], np.zeros((2, 3, 4)), _with(np.nan), _with(np.inf), _good()[:1], np.zeros((6, 0))):
        with pytest.raises(RuntimeError, match=r"^viscy_amd\.smoothness needs the HIP device \(no CPU fallback\)$"):
            smoothness.compute_embeddings_smoothness(types.SimpleNamespace(X=_as(kind, X), obs=obs))
        with pytest.raises(RuntimeError, match=r"^viscy_amd\.smoothness needs the HIP device \(no CPU fallback\)$"):
            smoothness.compute_track_displacement({"features": _as(kind, X), **obs})
    with pytest.raises(RuntimeError, match=r"^viscy_amd\.smoothness needs the HIP device \(no CPU fallback\)$"):
        smoothness.find_distribution_peak(np.linspace(0.0, 1.0, 50))
    with pytest.raises(ValueError, match="distance_metric"):     # what needs no data comes before the device
        smoothness.compute_embeddings_smoothness(types.SimpleNamespace(X=_as(kind, _good()), obs=obs), distance_metric="l1")


# ------------------------------------------------------------------------------------------------ the stratified draw
def _approximate_mode_restated(class_counts, n_draws, rng):
    """sklearn.utils.extmath._approximate_mode"""
    continuous = class_counts / class_counts.sum() * n_draws
    floored = np.floor(continuous)
    need = int(n_draws - floored.sum())
    ties = 0
    if need > 0:
        remainder = continuous - floored
        for value in np.sort(np.unique(remainder))[::-1]:
            (inds,) = np.where(remainder == value)
            add = min(len(inds), need)
            ties += len(inds) > add
            inds = rng.choice(inds, size=add, replace=False)
            floored[inds] += 1
            need -= add
            if need == 0:
                break
    return floored.astype(int), ties


def _shuffle_split_restated(y, n_train, n_test, rng):
    """one draw of sklearn's StratifiedShuffleSplit._iter_indices without its closing permutations -> (train, test, ties broken)"""
    classes, y_idx = np.unique(y, return_inverse=True)
    counts = np.bincount(y_idx)
    class_indices = np.split(np.argsort(y_idx, kind="mergesort"), np.cumsum(counts)[:-1])
    n_i, ties_a = _approximate_mode_restated(counts, n_train, rng)
    t_i, ties_b = _approximate_mode_restated(counts - n_i, n_test, rng)
    train, test = [], []
    for i in range(len(classes)):
        perm = class_indices[i].take(rng.permutation(counts[i]), mode="clip")
        train.extend(perm[: n_i[i]])
        test.extend(perm[n_i[i]: n_i[i] + t_i[i]])
    return train, test, ties_a + ties_b


def _labels(n, k):
    return np.random.RandomState(100 * n + k).permutation(np.arange(n) % k)   # every class has at least n // k >= 3 rows


SPLIT_CASES = [(n, k, f) for n in (9, 10, 37) for k in (2, 3) for f in (0.2, 0.3, 0.5, 0.8)]
SEEDS = (0, 1, 2, 7, 42)


def _same_state(a, b):
    sa, sb = a.get_state(), b.get_state()
    return sa[0] == sb[0] and np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]


@pytest.mark.parametrize("n,k,frac", SPLIT_CASES)
def test_the_shared_draw_and_both_wrappers_equal_the_restatement(n, k, frac):
    from viscy_amd import evalkit

    y = _labels(n, k)
    # the holdout of the validation callback: n_test = ceil(test_size n)
    n_test = int(math.ceil(frac * n))
    n_train = n - n_test
    for seed in SEEDS:
        if min(n_train, n_test) < k:
            with pytest.raises(ValueError, match=rf"^train \({n_train}\) and test \({n_test}\) parts must each hold at least one row per class \({k}\)$"):
                OE.stratified_holdout_ids(y, frac, seed)
            continue
        want = np.random.RandomState(seed)
        train, test, _ = _shuffle_split_restated(y, n_train, n_test, want)
        got = np.random.RandomState(seed)
        g_train, g_test = evalkit.stratified_shuffle_parts(y, n_train, n_test, got)
        assert isinstance(g_train, list) and isinstance(g_test, list)
        assert [int(i) for i in g_train] == [int(i) for i in train] and [int(i) for i in g_test] == [int(i) for i in test]
        assert _same_state(got, want)
        ids = np.zeros(n, dtype=np.int64)
        ids[test] = 1
        out = OE.stratified_holdout_ids(y, frac, seed)
        assert out.dtype == np.int64
        np.testing.assert_array_equal(out, ids)
    # train_test_split(train_size=) of the linear classifier: n_train = floor(train_size n), and one permutation of each part
    n_train = int(np.floor(frac * n))
    n_test = n - n_train
    for seed in SEEDS:
        if min(n_train, n_test) < k:
            with pytest.raises(ValueError, match=rf"^train \({n_train}\) and test \({n_test}\) parts must each hold at least one row per class \({k}\)$"):
                LC.stratified_split(y, frac, seed)
            continue
        want = np.random.RandomState(seed)
        train, test, _ = _shuffle_split_restated(y, n_train, n_test, want)
        train, test = want.permutation(train), want.permutation(test)
        g_train, g_test = LC.stratified_split(y, frac, seed)
        np.testing.assert_array_equal(g_train, train)
        np.testing.assert_array_equal(g_test, test)
        assert sorted(np.concatenate((g_train, g_test)).tolist()) == list(range(n))


def test_the_case_table_holds_a_tie_that_the_generator_breaks():
    y = _labels(10, 2)                      # 5 and 5 rows: 5 draws are 2.5 a class, and rng.choice decides which gets the third
    assert np.bincount(y).tolist() == [5, 5] and (10, 2, 0.5) in SPLIT_CASES
    sizes = set()
    for seed in range(8):
        train, _, ties = _shuffle_split_restated(y, 5, 5, np.random.RandomState(seed))
        assert ties >= 1
        sizes.add(int(np.sum(y[train] == 0)))
        got = LC.stratified_split(y, 0.5, seed)[0]
        assert int(np.sum(y[got] == 0)) == int(np.sum(y[train] == 0))
    assert sizes == {2, 3}                  # the draw matters: both answers occur among the seeds


def test_the_wrappers_keep_their_own_refusals():
    y = np.array([0, 0, 0, 1, 1, 1, 2])
    with pytest.raises(ValueError, match=r"^The least populated class has only 1 member: a stratified holdout needs 2 per class$"):
        OE.stratified_holdout_ids(y, 0.5)
    with pytest.raises(ValueError, match=r"^The least populated class in y has only 1 member, which is too few\.$"):
        LC.stratified_split(y, 0.5, 0)
    with pytest.raises(ValueError, match=r"^train_size=0\.01 leaves an empty part of 6 rows$"):
        LC.stratified_split(y[:6], 0.01, 0)
    with pytest.raises(ValueError, match=r"^train_size=1\.0 leaves an empty part of 6 rows$"):
        LC.stratified_split(y[:6], 1.0, 0)


def test_approximate_mode_and_average_ranks_are_one_function_each():
    from viscy_amd import evalkit

    assert OE.average_ranks is evalkit.average_ranks and LC.average_ranks is evalkit.average_ranks
    for counts, draws in (([5, 5], 5), ([4, 4, 4], 7), ([7, 2, 1], 4), ([3, 3], 6)):
        for seed in range(4):
            want, _ = _approximate_mode_restated(np.array(counts), draws, np.random.RandomState(seed))
            np.testing.assert_array_equal(evalkit.approximate_mode(np.array(counts), draws, np.random.RandomState(seed)), want)


# ------------------------------------------------------------------------------------------------ the two-row padding
@pytest.mark.parametrize("rows", (1, 2, 3))
def test_padded_to_two_rows(rows):
    from viscy_amd import evalkit

    x = torch.arange(rows * 4, dtype=torch.float32).reshape(rows, 4)
    x2, n = evalkit.padded_to_two_rows(x)
    assert n == rows
    if rows == 1:
        assert x2.shape == (2, 4) and torch.equal(x2[0], x[0]) and torch.equal(x2[1], x[0]) and torch.equal(x2[:n], x)
    else:
        assert x2 is x


# ------------------------------------------------------------------------------------------------ the source
def test_no_module_imports_a_private_name_of_a_sibling():
    root = pathlib.Path(reduce.__file__).parent
    found = []
    for path in sorted(root.rglob("*.py")):
        for node in ast.walk(ast.parse(path.read_text())):
            if isinstance(node, ast.ImportFrom) and node.level >= 1 and node.module:      # from .<module> import <names>
                found += [f"{path.relative_to(root)}:{node.lineno} from {'.' * node.level}{node.module} import {a.name}"
                          for a in node.names if a.name.startswith("_")]
    assert not found, "\n".join(found)


def test_evalkit_does_not_load_the_kernel_library_on_import():
    src = (pathlib.Path(reduce.__file__).parent / "evalkit.py").read_text()
    tree = ast.parse(src)
    top = [n for n in tree.body if isinstance(n, (ast.Import, ast.ImportFrom))]
    names = {a.name for n in top for a in n.names} | {n.module for n in top if isinstance(n, ast.ImportFrom)}
    assert "ops" not in names and "_lib" not in names
