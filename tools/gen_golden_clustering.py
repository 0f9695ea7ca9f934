"""Writes tests/golden/clustering.pt: what the reference's clustering.py (torch float64 distances; sklearn DBSCAN,
KNeighborsClassifier, normalized_mutual_info_score, adjusted_rand_score) gives on the fixtures of tests/ref_clustering.py.  Needs
scipy and sklearn; the tests do not: they read the golden.

    python tools/gen_golden_clustering.py <reference checkout>/packages/viscy-utils/src/viscy_utils/evaluation

clustering.py is loaded by path with `viscy_utils.tensor_utils` stubbed (a two-line to_numpy), as gen_golden_smoothness.py does.
Results only, no inputs: the fixtures are rebuilt from seeds.
  dist[name][metric]   pairwise_distance_matrix(x, metric, device="cpu"), float64 (N, N)
  ranks[name]          rank_nearest_neighbors of the Euclidean matrix: "raw" (normalize=False) and "norm"
  dbscan[name]         dbscan_clustering(x, eps, min_samples) labels, int64
  eval[name]           clustering_evaluation(x, the noisy blob labels, method) for "nmi" and "ari" (DBSCAN's defaults)
  knn[name]            knn_accuracy(x, y, k)
  scores               [(NMI, ARI)] of sklearn on ref_clustering.random_labelings()
  errors               (type name, message) of an unknown method and of k > N
  seeds                the seed the blob builder settled on per d"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import ref_clustering as RC  # noqa: E402


def load_reference(folder):
    for name in ("viscy_utils", "viscy_utils.tensor_utils"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["viscy_utils.tensor_utils"].to_numpy = lambda t: t.detach().cpu().numpy()
    spec = importlib.util.spec_from_file_location("reference_clustering", os.path.join(folder, "clustering.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def caught(fn):
    try:
        fn()
    except Exception as e:  # noqa: BLE001 - the type is what is recorded
        return (type(e).__name__, str(e))
    return None


def main():
    import scipy
    import sklearn
    from sklearn.metrics import adjusted_rand_score, normalized_mutual_info_score

    ref = load_reference(sys.argv[1])
    t = torch.from_numpy
    out = {"numpy": np.__version__, "scipy": scipy.__version__, "sklearn": sklearn.__version__, "torch": torch.__version__,
           "dist": {}, "ranks": {}, "dbscan": {}, "eval": {}, "knn": {}}
    for name in RC.DISTANCE_CASES:
        x = RC.distance_case(name)
        out["dist"][name] = {m: t(np.ascontiguousarray(ref.pairwise_distance_matrix(x, metric=m, device="cpu"))) for m in ("cosine", "euclidean")}
        if name in RC.RANK_CASES:
            eu = out["dist"][name]["euclidean"].numpy()
            out["ranks"][name] = {"raw": t(np.ascontiguousarray(ref.rank_nearest_neighbors(eu, normalize=False)).astype(np.int64)),
                                  "norm": t(np.ascontiguousarray(ref.rank_nearest_neighbors(eu, normalize=True)))}
        print(f"dist {name}: {x.shape}, max |d_ii| euclidean {np.abs(np.diag(out['dist'][name]['euclidean'].numpy())).max():.3e}")
    for name, (x, eps, min_samples) in RC.dbscan_cases().items():
        labels = np.asarray(ref.dbscan_clustering(x, eps=eps, min_samples=min_samples)).astype(np.int64)
        out["dbscan"][name] = t(labels)
        print(f"dbscan {name}: {x.shape} eps {eps} min_samples {min_samples}: {labels.max() + 1} clusters, {(labels < 0).sum()} noise")
    out["seeds"] = {}
    for d in (16, 768):
        seed, (x, _, y) = RC.blob_case(d)
        out["seeds"][d] = seed
        out["eval"]["blobs_%d" % d] = {m: float(ref.clustering_evaluation(x, y, method=m)) for m in ("nmi", "ari")}
        print(f"eval blobs_{d}: seed {seed}", out["eval"]["blobs_%d" % d])
    for name, (x, y, k) in RC.knn_cases().items():
        out["knn"][name] = float(ref.knn_accuracy(x, y, k=k))
        print(f"knn {name}: k {k} accuracy {out['knn'][name]:.6f}")
    out["scores"] = [(float(normalized_mutual_info_score(a, b)), float(adjusted_rand_score(a, b))) for a, b in RC.random_labelings()]
    x5 = RC.real_features(5, 4, 1)
    out["errors"] = {"method": caught(lambda: ref.clustering_evaluation(x5, np.arange(5), method="purity")),
                     "k_above_n": caught(lambda: ref.knn_accuracy(x5, np.arange(5) % 2, k=7))}
    print("errors:", out["errors"])
    path = os.path.join(ROOT, "tests", "golden", "clustering.pt")
    torch.save(out, path)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
