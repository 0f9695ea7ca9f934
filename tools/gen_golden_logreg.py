"""Writes tests/golden/logreg.pt: what sklearn's LogisticRegression, its splitters and metrics, and the reference's
train_linear_classifier / predict_with_classifier give on the fixtures of tests/ref_logreg.py.  Needs sklearn and pandas; the tests
do not: they read the golden.

    python tools/gen_golden_logreg.py <reference checkout>/packages/viscy-utils/src/viscy_utils/evaluation/linear_classifier.py

The reference module is loaded by path with its annotation import stubbed.  Results only, no inputs: the fixtures are rebuilt from
seeds.
  cases[name]     "tight": coef, intercept of the fit at tol=1e-10; "default": coef, intercept, pred (class indices), proba, decision
                  of the fit as the reference runs it (default tol); dist_tight / dist_default: per problem, the distance of either fit
                  from the float64 optimum u* of tests/ref_logreg.py in the coordinates [w; w_b]; undecided: the fraction of rows whose
                  label the default fit's error could change (asserted <= 2 %)
  splits[seed]    train_test_split(stratify) and GroupShuffleSplit indices, in order
  metrics[name]   classification_report(output_dict=True) and roc_auc_score on the metric fixtures
  pipeline[cfg]   the reference's metrics, val_outputs and, per AUROC key, |default-tol - tol=1e-10|; every row decided by 10 x the bound
                  (asserted)
  predict         the keys and NaN rows predict_with_classifier writes"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import ref_logreg as RL  # noqa: E402


def load_reference(path):
    for name in ("viscy_utils", "viscy_utils.evaluation", "viscy_utils.evaluation.annotation"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["viscy_utils.evaluation.annotation"].load_annotation_anndata = None
    spec = importlib.util.spec_from_file_location("reference_linear_classifier", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def distances(x64, y_idx, params, est):
    d = x64.shape[1]
    U = RL.stack_u(est.coef_, est.intercept_, params, d)
    out = []
    for prob, u in zip(RL.problems(params, y_idx), U):
        out.append(float(np.linalg.norm(u - RL.solve(x64, prob, params)[0])))
    return out


def main():
    import sklearn
    from sklearn.linear_model import LogisticRegression
    from sklearn.metrics import classification_report, roc_auc_score
    from sklearn.model_selection import GroupShuffleSplit, train_test_split

    ref = load_reference(sys.argv[1])
    out = {"cases": {}, "splits": {}, "metrics": {}, "pipeline": {}, "numpy": np.__version__, "sklearn": sklearn.__version__}

    for name, c in RL.CASES.items():
        x, y = RL.build(name)
        x64, params = x.astype(np.float64), c["params"]
        tight = LogisticRegression(**{**params, "tol": 1e-10, "max_iter": 100000}).fit(x, y)
        default = LogisticRegression(**params).fit(x, y)
        d_tight, d_default = distances(x64, y, params, tight), distances(x64, y, params, default)
        z = default.decision_function(x)
        undecided = float(np.mean(~RL.decided(z, RL.row_bound(x, max(d_default)))))
        print(f"{name}: |sk(1e-10) - u*| {max(d_tight):.2e}  |sk(default) - u*| {max(d_default):.2e}  undecided {undecided:.4f}  "
              f"|u*| {max(np.linalg.norm(o[0]) for o in RL.optimum(name)):.2f}")
        assert undecided <= RL.UNDECIDED_CAP, (name, undecided)
        t = torch.from_numpy
        out["cases"][name] = {
            "tight": {"coef": t(tight.coef_.copy()), "intercept": t(np.atleast_1d(tight.intercept_).astype(np.float64))},
            "default": {"coef": t(default.coef_.copy()), "intercept": t(np.atleast_1d(default.intercept_).astype(np.float64)),
                        "pred": t(default.predict(x).astype(np.int64)), "proba": t(default.predict_proba(x)), "decision": t(np.asarray(z))},
            "dist_tight": d_tight, "dist_default": d_default, "undecided": undecided}

    for seed in RL.SPLIT_SEEDS:
        y, groups = RL.split_labels(seed)
        idx = np.arange(len(y))
        tr, te = train_test_split(idx, train_size=0.8, random_state=seed, stratify=y, shuffle=True)
        gtr, gte = next(GroupShuffleSplit(n_splits=1, train_size=0.75, random_state=seed).split(idx, y, groups=groups))
        out["splits"][seed] = {"strat": (torch.from_numpy(tr), torch.from_numpy(te)), "group": (torch.from_numpy(gtr), torch.from_numpy(gte))}

    for name, (yt, yp, score) in RL.metric_fixtures().items():
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            rep = classification_report(yt, yp, digits=3, output_dict=True)
        entry = {"report": rep}
        if np.ndim(score) == 1:
            entry["auroc"] = float(roc_auc_score(yt, score))
        else:
            entry["auroc"] = float(roc_auc_score(yt, score, multi_class="ovr", average="macro"))
            entry["auroc_per_class"] = [float(roc_auc_score((yt == c).astype(int), score[:, i])) for i, c in enumerate(np.unique(yt))]
        out["metrics"][name] = entry

    x, y, groups, _ = RL.pipe_arrays()
    task = RL.pipe_task()
    for cfg, (scal, use_pca, k, grouped, frac) in RL.PIPE_CONFIGS.items():
        runs = {}
        for label, extra in (("default", {}), ("tight", {"tol": 1e-10, "max_iter": 100000})):
            runs[label] = ref.train_linear_classifier(RL.pipe_adata(), task, use_scaling=scal, use_pca=use_pca, n_pca_components=k,
                                                      classifier_params={**RL.PIPE_PARAMS, **extra}, split_train_data=frac, random_seed=42,
                                                      groups=groups if grouped else None)
        pipe, metrics, val = runs["default"]
        # every row decided by 10 x the bound: the count metrics of any fit as close to u* as sklearn's are sklearn's
        X = np.asarray(pipe.transform(np.array(x)), dtype=np.float64)
        idx = np.arange(len(y))
        if frac >= 1.0:
            tr, te = idx, idx[:0]
        elif grouped:
            tr, te = next(GroupShuffleSplit(n_splits=1, train_size=frac, random_state=42).split(idx, y, groups=groups))
        else:
            tr, te = train_test_split(idx, train_size=frac, random_state=42, stratify=y, shuffle=True)
        classes, y_idx = np.unique(y[tr], return_inverse=True)
        dist = max(distances(X[tr], y_idx, RL.PIPE_PARAMS, pipe.classifier))
        z = pipe.classifier.decision_function(X)
        ok = RL.decided(z, 10.0 * RL.row_bound(X, dist))
        print(f"pipeline {cfg}: |sk - u*| {dist:.2e}  rows not decided by 10 x the bound: {int((~ok).sum())}  val_accuracy "
              f"{metrics.get('val_accuracy')}  train_auroc {metrics['train_auroc']:.6f}")
        assert ok.all(), cfg
        if frac < 1.0:
            assert np.array_equal(val["y_val"], y[te])
        auroc_diff = {key: abs(metrics[key] - runs["tight"][1][key]) for key in metrics if key.endswith("auroc")}
        out["pipeline"][cfg] = {"metrics": {k_: float(v) for k_, v in metrics.items()}, "auroc_diff": auroc_diff, "classes": val["classes"],
                                "y_val": None if val["y_val"] is None else list(val["y_val"]),
                                "y_val_proba": None if val["y_val_proba"] is None else torch.from_numpy(np.asarray(val["y_val_proba"]))}

    pipe = runs["default"][0]   # "scaled_all"
    ad = ref.predict_with_classifier(RL.pipe_adata(), pipe, task, artifact_metadata={"artifact_name": "m:v3", "artifact_id": "id7",
                                                                                      "artifact_version": "v3"}, include_wells=["A/1", "B/2"])
    pred = ad.obs[f"predicted_{task}"]
    out["predict"] = {"obs_keys": sorted(ad.obs.columns), "obsm_keys": sorted(ad.obsm), "uns": dict(ad.uns),
                      "nan_rows": torch.from_numpy(np.flatnonzero(pred.isna().to_numpy())), "pred": [p if isinstance(p, str) else None for p in pred]}
    path = os.path.join(ROOT, "tests", "golden", "logreg.pt")
    torch.save(out, path)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
