"""CPU: the host side of viscy_amd.linear_classifier against sklearn's recorded results (tests/golden/logreg.pt).

newton_fit with the numpy evaluator of tests/ref_logreg.py reaches |g| <= eps |g(0)| on every case and lands as close to sklearn's
tol=1e-10 coefficients as that fit is to the float64 optimum u* (plus the solver's own distance from u*, |g| / lambda_min of the
Hessian: 1 for liblinear's objective): this pins the restatement of the objectives, the one-vs-rest cp / cn rule included.  The
splits equal sklearn's indices in order; the metrics equal classification_report and roc_auc_score to 1e-12; the class-weight rules
and every NotImplementedError."""

import functools
import warnings

import numpy as np
import pytest

from tests import ref_logreg as RL
from tests.conftest import load_golden


@functools.lru_cache(maxsize=None)
def golden():
    return load_golden("logreg.pt")


def numpy_fit(name):
    from viscy_amd.linear_classifier import LogisticRegression, newton_fit

    x, y = RL.build(name)
    x64, params = x.astype(np.float64), RL.CASES[name]["params"]
    est = LogisticRegression(**params)
    classes, y_idx = np.unique(y, return_inverse=True)
    out = []
    for (pos, cp, cn), prob in zip(est.problems(classes, y_idx), RL.problems(params, y)):
        assert np.array_equal(prob[1], np.where(y_idx == pos, cp, cn))     # the two statements of the rule agree
        res = newton_fit(lambda w, b, h, prob=prob: RL.data_terms(x64, prob[0], prob[1], w, b, h), x.shape[1],
                         penalised_intercept=params["solver"] == "liblinear", intercept_scaling=1.0,
                         tol=est.tolerance(prob[2], len(y)), max_iter=params["max_iter"], fit_intercept=params.get("fit_intercept", True))
        out.append((res, prob))
    return x64, params, out


@pytest.mark.parametrize("name", list(RL.CASES))
def test_newton_fit_reaches_the_optimum_of_sklearns_objective(name):
    x64, params, fits = numpy_fit(name)
    g = golden()["cases"][name]
    U_sk = RL.stack_u(g["tight"]["coef"].numpy(), g["tight"]["intercept"].numpy(), params, x64.shape[1])
    for k, (res, prob) in enumerate(fits):
        u_star, g0, lam, eps = RL.optimum(name)[k]
        assert eps == RL.epsilon(params, prob[2], len(x64)) <= 1e-10
        grad = RL.gradient(x64, prob, params, res.w, res.b)
        gn = float(np.linalg.norm(grad))
        print(f"\n{name}[{k}]: {res.n_iter} iterations, {res.n_evals} trials, |g| / |g(0)| = {gn / g0:.2e} (eps {eps:.1e}), "
              f"lambda_min {lam:.3f}, |u - u*| {np.linalg.norm(RL.stack_u(res.w, [res.b], params, x64.shape[1])[0] - u_star):.2e}, "
              f"|sk - u*| {g['dist_tight'][k]:.2e}")
        assert res.converged and res.grad_norm0 == pytest.approx(g0, rel=1e-12)
        assert gn <= eps * g0
        u = RL.stack_u(res.w, [res.b], params, x64.shape[1])[0]
        # the objective is lambda_min-strongly convex near u*: |u - u*| <= 2 |g| / lambda_min (2: the Hessian between u and u*)
        own = 2.0 * gn / min(lam, 1.0) if params["solver"] != "liblinear" else gn
        if params["solver"] == "liblinear":
            assert lam >= 1.0 - 1e-9
        assert np.linalg.norm(u - u_star) <= own + 1e-14 * np.linalg.norm(u_star)
        assert np.linalg.norm(u - U_sk[k]) <= g["dist_tight"][k] + own + 1e-14 * np.linalg.norm(u_star)


def test_newton_fit_warns_when_the_iterations_run_out():
    from viscy_amd.linear_classifier import newton_fit

    x, y = RL.build("bin_n300_d132_bal")
    x64 = x.astype(np.float64)
    prob = RL.problems(RL.CASES["bin_n300_d132_bal"]["params"], y)[0]
    with pytest.warns(RuntimeWarning, match="2 Newton iterations"):
        res = newton_fit(lambda w, b, h: RL.data_terms(x64, prob[0], prob[1], w, b, h), 132, tol=1e-10, max_iter=2)
    assert not res.converged and res.n_iter == 2


@pytest.mark.parametrize("seed", RL.SPLIT_SEEDS)
def test_splits_equal_sklearns_indices_in_order(seed):
    from viscy_amd.linear_classifier import group_shuffle_split, stratified_split

    y, groups = RL.split_labels(seed)
    g = golden()["splits"][seed]
    tr, te = stratified_split(y, 0.8, seed)
    assert np.array_equal(tr, g["strat"][0].numpy()) and np.array_equal(te, g["strat"][1].numpy())
    gtr, gte = group_shuffle_split(groups, 0.75, seed)
    assert np.array_equal(gtr, g["group"][0].numpy()) and np.array_equal(gte, g["group"][1].numpy())
    assert not set(groups[gtr]) & set(groups[gte])


def test_metrics_equal_sklearns():
    from viscy_amd.linear_classifier import _auroc, classification_report, roc_auc

    for name, (yt, yp, score) in RL.metric_fixtures().items():
        g = golden()["metrics"][name]
        rep = classification_report(yt, yp)
        assert set(rep) == set(g["report"])
        for key, want in g["report"].items():
            if key == "accuracy":
                assert abs(rep[key] - want) <= 1e-12
            else:
                for m, v in want.items():
                    assert abs(rep[key][m] - v) <= 1e-12, (name, key, m)
        classes = np.unique(yt)
        if np.ndim(score) == 1:
            assert abs(roc_auc(yt == classes[1], score) - g["auroc"]) <= 1e-12
            assert abs(_auroc(yt, np.stack((1 - score, score), axis=1), classes) - g["auroc"]) <= 1e-12
        else:
            assert abs(_auroc(yt, score, classes) - g["auroc"]) <= 1e-12
            for i, c in enumerate(classes):
                assert abs(roc_auc(yt == c, score[:, i]) - g["auroc_per_class"][i]) <= 1e-12
    assert golden()["metrics"]["three_absent"]["report"]["c"]["precision"] == 0.0     # the class absent from the predictions
    with pytest.raises(ValueError, match="Only one class"):
        roc_auc(np.ones(5, dtype=bool), np.arange(5.0))
    with pytest.raises(ValueError, match="Number of classes"):
        _auroc(np.array(["a", "b"] * 3, dtype=object), np.full((6, 3), 1 / 3), np.array(["a", "b", "c"], dtype=object))


def test_class_weight_rules():
    from viscy_amd.linear_classifier import LogisticRegression, class_weights

    classes, y_idx = np.array(["a", "b", "c"], dtype=object), np.array([0, 0, 0, 1, 1, 2])
    assert np.array_equal(class_weights(None, classes, y_idx), np.ones(3))
    assert np.allclose(class_weights("balanced", classes, y_idx), 6 / (3 * np.array([3.0, 2.0, 1.0])), rtol=0, atol=0)
    assert np.array_equal(class_weights({"b": 2.5}, classes, y_idx), [1.0, 2.5, 1.0])
    with pytest.raises(ValueError, match="not in"):
        class_weights({"z": 2.0}, classes, y_idx)
    with pytest.raises(ValueError, match="balanced"):
        class_weights("auto", classes, y_idx)
    est = LogisticRegression(solver="liblinear", C=2.0, class_weight="balanced")
    assert est.problems(classes, y_idx) == [(0, 2.0 * 6 / 9, 2.0), (1, 2.0 * 6 / 6, 2.0), (2, 2.0 * 6 / 3, 2.0)]    # the rest class: C alone
    two, idx2 = classes[:2], np.array([0, 0, 0, 1])
    assert est.problems(two, idx2) == [(1, 2.0 * 4 / 2, 2.0 * 4 / 6)]
    assert LogisticRegression(tol=1e-4).tolerance(10, 100) == 1e-10 and LogisticRegression(tol=1e-12).tolerance(10, 100) == 1e-12 * 10 / 100


@pytest.mark.parametrize("kwargs,classes,match", [
    (dict(solver="lbfgs"), 3, "multinomial"),
    (dict(solver="saga", penalty="l1"), 2, "penalty='l1'"),
    (dict(solver="saga", penalty="elasticnet", l1_ratio=0.5), 2, "penalty='elasticnet'"),
    (dict(penalty=None), 2, "penalty=None"),
    (dict(l1_ratio=0.3), 2, "l1_ratio=0.3"),
    (dict(solver="liblinear", dual=True), 2, "dual=True"),
    (dict(warm_start=True), 2, "warm_start"),
    (dict(multi_class="multinomial"), 2, "multi_class='multinomial'"),
])
def test_what_is_not_served_says_so(kwargs, classes, match):
    from viscy_amd.linear_classifier import LogisticRegression

    with pytest.raises(NotImplementedError, match=match):
        LogisticRegression(**kwargs)._check_served(classes, None)


def test_sample_weight_and_bad_arguments():
    from viscy_amd.linear_classifier import LogisticRegression

    x = np.zeros((4, 3), dtype=np.float32)
    with pytest.raises(NotImplementedError, match="sample_weight"):
        LogisticRegression().fit(x, [0, 1, 0, 1], sample_weight=np.ones(4))
    with pytest.raises(ValueError, match="only one class"):
        LogisticRegression().fit(x, [1, 1, 1, 1])
    with pytest.raises(ValueError, match="solver='newton'"):
        LogisticRegression(solver="newton").fit(x, [0, 1, 0, 1])
    with pytest.raises(ValueError, match="one label per row"):
        LogisticRegression().fit(x, [0, 1])
    with pytest.raises(NotImplementedError, match="d=5000"):
        LogisticRegression().fit(np.zeros((4, 5000), dtype=np.float32), [0, 1, 0, 1])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        LogisticRegression(solver="liblinear")._check_served(3, None)     # one-vs-rest is served


def test_the_entry_points_refuse_bad_arguments_before_any_launch():
    import ctypes

    from viscy_amd import _lib

    l = _lib.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    big = 1 << 40
    for n, d in ((1, 4), (1 << 31, 4), (8, 0), (8, 4097)):
        assert l.vsx_logreg_rows_ws_bytes(n, d) == 0 and l.vsx_wcolsum_ws_bytes(n, d, 2) == 0
        assert l.vsx_logreg_rows(p, n, d, p, 0.0, p, 1, 1.0, 1.0, p, p, p, p, p, p, big, None) == 1 and b"must be in" in l.vsx_last_error()
        assert l.vsx_wcolsum(p, n, d, p, 2, p, p, big, None) == 1 and b"must be in" in l.vsx_last_error()
        assert l.vsx_gram_scaled(p, n, d, None, p, p, p, big, None) == 1 and b"vsx_gram_scaled" in l.vsx_last_error()
    assert l.vsx_wcolsum_ws_bytes(8, 4, 0) == 0 and l.vsx_wcolsum_ws_bytes(8, 4, 5) == 0 and l.vsx_wcolsum_ws_bytes(8, 4, 4) == 4 * 4 * 8
    assert l.vsx_logreg_rows_ws_bytes(8, 4) == 24 and l.vsx_logreg_rows_ws_bytes(10 ** 6, 768) == 2033 * 24    # runs of 492 rows
    for args, msg in (((p, 8, 4, p, 5, p, p, big, None), b"m=5 must be in [1, 4]"), ((p, 8, 4, None, 2, p, p, big, None), b"null argument"),
                      ((p + 2, 8, 4, p, 2, p, p, big, None), b"4-byte aligned"), ((p, 8, 4, p, 2, p + 4, p, big, None), b"8-byte aligned"),
                      ((p, 8, 4, p, 2, p, p, 63, None), b"bytes (got 63)")):
        assert l.vsx_wcolsum(*args) == 1 and msg in l.vsx_last_error(), l.vsx_last_error()
    rows = lambda **k: l.vsx_logreg_rows(*[k.get(a, v) for a, v in (("x", p), ("n", 8), ("d", 4), ("w", p), ("b", 0.0), ("labels", p), ("pos", 1),
                                                                      ("cp", 1.0), ("cn", 1.0), ("z", p), ("r", p), ("s", p), ("q", p),
                                                                      ("sums", p), ("ws", p), ("ws_bytes", big), ("stream", None))])
    for kw, msg in ((dict(w=None), b"null argument"), (dict(labels=None), b"labels are needed"), (dict(ws=None), b"need a workspace"),
                    (dict(z=None, r=None, s=None, q=None, sums=None), b"null argument"), (dict(x=p + 2), b"4-byte aligned"),
                    (dict(r=p + 4), b"8-byte aligned"), (dict(ws_bytes=23), b"bytes (got 23)")):
        assert rows(**kw) == 1 and msg in l.vsx_last_error(), (kw, l.vsx_last_error())
    for args, msg in (((p, 8, 4, None, None, p, p, big, None), b"null argument"), ((p, 8, 4, p, p, None, p, big, None), b"null argument"),
                      ((p, 8, 4, None, p + 2, p, p, big, None), b"4-byte aligned"), ((p, 8, 4, p, p, p, p, 100, None), b"bytes (got 100)")):
        assert l.vsx_gram_scaled(*args) == 1 and msg in l.vsx_last_error() and b"vsx_gram_scaled" in l.vsx_last_error(), l.vsx_last_error()
