"""Writes tests/golden/online_eval.pt: what sklearn, scipy and the reference's online_eval.py give on the case table of
tests/ref_online_eval.py.  Needs scikit-learn and scipy (the GPU tests do not: they read the golden).

    python tools/gen_golden_online_eval.py <reference checkout>/packages/viscy-utils/src/viscy_utils/callbacks/online_eval.py \\
        [<reference checkout>/applications/dynaclr/configs/training/DynaCLR-2D/DynaCLR-2D-BagOfChannels-v3.yml]

The reference module is loaded by path, with stub modules for what it imports but the three functions used here never touch
(lightning, lightning_utilities, viscy_data._typing, viscy_utils.tensor_utils).  Inputs are not stored: the table rebuilds them
from seeds.  Per k-NN case: sklearn's score (``cross_val_score(...).mean()`` or the holdout score), its per-row predictions
(``cross_val_predict``; -1 outside the holdout's test part), the fold ids / holdout ids, and the per-row "undecided" mask of the
float64 restatement (ref_online_eval.undecided) — asserted here to cover at most 2 % of the rows.  Per effective-rank and
smoothness case: the reference's value on the fp32 input and on the input cast to float64, and the margin
4 |fp32 - fp64| + 1e-9 the tests allow.  The smoothness cases also carry the reference loop's pair order and scipy's ranks.
With a recipe path: the ``trainer.callbacks`` list of that YAML file, as parsed."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import ref_online_eval as RO  # noqa: E402


def load_reference(path):
    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    stub("lightning")
    stub("lightning.pytorch", LightningModule=object, Trainer=object)
    stub("lightning.pytorch.callbacks", Callback=object)
    stub("lightning_utilities")
    stub("lightning_utilities.core")
    stub("lightning_utilities.core.rank_zero", rank_zero_warn=lambda *a, **k: None)
    stub("viscy_data")
    stub("viscy_data._typing", TripletSample=dict)
    stub("viscy_utils")
    stub("viscy_utils.tensor_utils", to_numpy=lambda t: t.detach().cpu().numpy())
    spec = importlib.util.spec_from_file_location("reference_online_eval", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def margin(v32, v64):
    return 4.0 * abs(v32 - v64) + 1e-9


def main():
    import scipy
    import sklearn
    from scipy.stats import rankdata, spearmanr
    from sklearn.model_selection import StratifiedKFold, cross_val_predict, cross_val_score, train_test_split
    from sklearn.neighbors import KNeighborsClassifier

    ref = load_reference(sys.argv[1])
    out = {"knn": {}, "erank": {}, "smooth": {}, "sklearn": sklearn.__version__, "scipy": scipy.__version__}
    for name, c in RO.KNN_CASES.items():
        x, y = RO.build_knn(name)
        k = min(c["k"], c["N"] - 1)
        knn = KNeighborsClassifier(n_neighbors=k, metric="cosine")
        if c["mode"] == "cv":
            folds = min(5, int(np.bincount(y).min()))
            acc = float(cross_val_score(knn, x, y, cv=folds).mean())
            pred = cross_val_predict(knn, x, y, cv=folds)
            group = np.empty(len(y), dtype=np.int64)
            for f, (_, test) in enumerate(StratifiedKFold(folds).split(x, y)):
                group[test] = f
            scored = np.ones(len(y), dtype=bool)
            entry = {"folds": folds}
        else:
            rows = np.arange(len(y))
            x_tr, x_te, y_tr, y_te, r_tr, r_te = train_test_split(x, y, rows, test_size=RO.HOLDOUT_TEST_SIZE, stratify=y, random_state=0)
            knn.fit(x_tr, y_tr)
            acc = float(knn.score(x_te, y_te))
            pred = np.full(len(y), -1, dtype=np.int64)
            pred[r_te] = knn.predict(x_te)
            group = np.zeros(len(y), dtype=np.int64)
            group[r_te] = 1
            scored = group == 1
            entry = {"test_rows": torch.from_numpy(r_te.copy()), "train_rows": torch.from_numpy(r_tr.copy())}
        ours, und = RO.undecided(x, y, group, k)
        share = und[scored].mean()
        differ = int(((ours != pred) & scored).sum())
        differ_decided = int(((ours != pred) & scored & ~und).sum())
        print(f"{name:24s} sklearn acc {acc:.6f}  undecided {int(und[scored].sum())}/{int(scored.sum())} ({100 * share:.2f} %)  "
              f"restatement differs from sklearn on {differ} rows ({differ_decided} of them decided)")
        assert share <= 0.02, (name, share)
        assert differ_decided == 0, name
        entry.update(acc=acc, k=k, pred=torch.from_numpy(pred.astype(np.int64)), group=torch.from_numpy(group),
                     undecided=torch.from_numpy(und))
        out["knn"][name] = entry
    for name in RO.ERANK_CASES:
        x, _ = RO.build_knn(name)
        v32, v64 = ref.effective_rank(x), ref.effective_rank(x.astype(np.float64))
        out["erank"][name] = {"fp32": v32, "fp64": v64, "margin": margin(v32, v64)}
        print(f"effective_rank {name}: fp64 {v64:.12f}  |fp32 - fp64| {abs(v32 - v64):.3e}")
    for name in RO.SMOOTH_CASES:
        x, tid, t = RO.build_smooth(name)
        v32, v64 = ref.temporal_smoothness(x, tid, t), ref.temporal_smoothness(x.astype(np.float64), tid, t)
        pi, pj = RO.track_pairs_loop(tid)
        x64 = x.astype(np.float64)
        xn = x64 / (np.linalg.norm(x64, axis=1, keepdims=True) + 1e-10)
        d64 = 1.0 - (xn[pi] * xn[pj]).sum(1)
        dt = np.abs(t[pi] - t[pj]).astype(np.float64)
        entry = {"fp32": v32, "fp64": v64, "margin": margin(v32, v64) if not np.isnan(v64) else float("nan"),
                 "pi": torch.from_numpy(pi), "pj": torch.from_numpy(pj), "dist64": torch.from_numpy(d64)}
        if len(pi) >= 3:
            entry.update(rank_dt=torch.from_numpy(rankdata(dt)), rank_dist=torch.from_numpy(rankdata(d64)),
                         rho_scipy=float(spearmanr(dt, d64)[0]))
        out["smooth"][name] = entry
        print(f"temporal_smoothness {name}: {len(pi)} pairs  fp64 {v64:.12f}  |fp32 - fp64| {abs(v32 - v64):.3e}")
    if len(sys.argv) > 2:
        import yaml

        with open(sys.argv[2]) as f:
            out["recipe"] = {"file": os.path.basename(sys.argv[2]), "callbacks": yaml.safe_load(f)["trainer"]["callbacks"]}
        print("recipe callbacks:", [c["class_path"] for c in out["recipe"]["callbacks"]])
    path = os.path.join(ROOT, "tests", "golden", "online_eval.pt")
    torch.save(out, path)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
