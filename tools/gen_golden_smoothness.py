"""Writes tests/golden/smoothness.pt: what the reference's compute_embeddings_smoothness / find_distribution_peak (scipy cdist,
gaussian_kde, find_peaks; sklearn StandardScaler) and the loop of its compute_track_displacement give on the fixtures of
tests/ref_smoothness.py.  Needs scipy, sklearn and pandas; the tests do not: they read the golden.

    python tools/gen_golden_smoothness.py <reference checkout>/packages/viscy-utils/src/viscy_utils/evaluation

smoothness.py and clustering.py are loaded by path; `anndata` and `viscy_utils.tensor_utils` are stubbed (the latter with a
two-line to_numpy) and a small object with .X and .obs stands in for the AnnData.  compute_track_displacement itself needs
xarray, so its loop is restated here around the reference's own pairwise_distance_matrix(device="cpu") and compare_time_offset.
Results only, no inputs: the fixtures are rebuilt from seeds.
  cases[name]     stats; adjacent / random (float64; case C: every 16th value as *_s16 and values 9936 .. 10063 as *_mid);
                  piecewise (C: piecewise_lengths only); mean_, scale_ of sklearn's StandardScaler; z = its fit_transform (cases of
                  at most 64 rows); redraws = passes of the i == j loop, counted on the reference's own np.random.randint calls; error = (type name, message) where the reference raises
  curves          case A: gaussian_kde on linspace(min, max, 1000) for either distribution, and the histogram-method peaks
  msd[metric]     [(tau, [distances])] in the dict's insertion order
  find_peaks      scipy.signal.find_peaks(y, height=0.1 max y) indices for the signals of ref_smoothness.peak_signals() and the two curves
  errors          find_distribution_peak on the degenerate samples and an unknown method: (type name, message)"""
import importlib.util
import os
import sys
import types
from collections import defaultdict

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import ref_smoothness as RS  # noqa: E402


def load_reference(folder):
    for name in ("anndata", "viscy_utils", "viscy_utils.tensor_utils"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["anndata"].AnnData = object
    sys.modules["viscy_utils.tensor_utils"].to_numpy = lambda t: t.detach().cpu().numpy()
    mods = []
    for stem in ("smoothness", "clustering"):
        spec = importlib.util.spec_from_file_location("reference_" + stem, os.path.join(folder, stem + ".py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mods.append(mod)
    return mods


def caught(fn):
    try:
        fn()
    except Exception as e:  # noqa: BLE001 - the type is what is recorded
        return (type(e).__name__, str(e))
    return None


def track_displacement(clustering, ds, metric):
    """distance.py:compute_track_displacement with the xarray selections written as masks"""
    import pandas as pd

    tracks = pd.DataFrame({"fov_name": ds["fov_name"], "track_id": ds["track_id"]}).drop_duplicates()
    out = defaultdict(list)
    for fov_name, track_id in zip(tracks["fov_name"], tracks["track_id"]):
        sel = (ds["fov_name"] == fov_name) & (ds["track_id"] == track_id)
        t, feats = ds["t"][sel], ds["features"][sel]
        order = np.argsort(t)
        times, emb = t[order], feats[order]
        dm = clustering.pairwise_distance_matrix(emb, metric=metric, device="cpu")
        for off in range(1, len(times)):
            for i, disp in enumerate(clustering.compare_time_offset(dm, off)):
                out[int(times[i + off] - times[i])].append(float(disp))
    return dict(out)


def main():
    import scipy
    import sklearn
    from scipy.stats import gaussian_kde
    from sklearn.preprocessing import StandardScaler

    smooth, clustering = load_reference(sys.argv[1])
    t = torch.from_numpy
    out = {"cases": {}, "numpy": np.__version__, "scipy": scipy.__version__, "sklearn": sklearn.__version__}
    for name in RS.CASES:
        ad, metric, offsets = RS.adata(name, frame=True)
        n = len(ad.X)
        sc = StandardScaler().fit(ad.X)
        entry = {"mean_": t(sc.mean_.copy()), "scale_": t(sc.scale_.copy())}
        if n <= 64:
            entry["z"] = t(StandardScaler().fit_transform(ad.X))
        state = np.random.get_state()
        res, draws, randint = [], [0], np.random.randint

        def counting(*a, **k):      # the reference draws through np.random.randint: two calls per batch, one more per redraw pass
            draws[0] += 1
            return randint(*a, **k)

        np.random.randint = counting
        try:
            entry["error"] = caught(lambda: res.append(smooth.compute_embeddings_smoothness(ad, distance_metric=metric, time_offsets=offsets)))
        finally:
            np.random.randint = randint
        np.random.set_state(state)
        if res:
            stats, dist, piecewise = res[0]
            adj, rnd = dist["adjacent_frame_distribution"], dist["random_frame_distribution"]
            entry["stats"] = {k: float(v) for k, v in stats.items()}
            entry["piecewise_lengths"] = [len(p) for p in piecewise]
            entry["redraws"] = draws[0] - 2 * -(-len(adj) // 10000)
            if name == "C":
                for key, v in (("adjacent", adj), ("random", rnd)):
                    entry[key + "_s16"], entry[key + "_mid"] = t(v[::16].copy()), t(v[9936:10064].copy())
                entry["n_pairs"] = len(adj)
            else:
                entry["adjacent"], entry["random"] = t(adj.copy()), t(rnd.copy())
                entry["piecewise"] = [[float(v) for v in p] for p in piecewise]
            print(f"{name}: N {n}, {len(adj)} pairs, redraw passes {entry['redraws']}, " + ", ".join(f"{k} {v:.6g}" for k, v in stats.items()))
            if name == "A":
                out["curves"] = {}
                for key, v in (("adjacent", adj), ("random", rnd)):
                    grid = np.linspace(np.min(v), np.max(v), 1000)
                    out["curves"][key] = t(gaussian_kde(v)(grid))
                    out["curves"][key + "_hist_peak"] = float(smooth.find_distribution_peak(v, method="histogram"))
        else:
            print(f"{name}: N {n}, raises {entry['error']}")
        out["cases"][name] = entry

    from scipy.signal import find_peaks

    def peaks(y):
        return find_peaks(y, height=0.1 * np.max(y))[0].tolist()

    out["find_peaks"] = {"signals": [peaks(y) for y in RS.peak_signals()], "curves": {k: peaks(out["curves"][k].numpy()) for k in ("adjacent", "random")}}
    ds = RS.msd_dataset()
    out["msd"] = {metric: list(track_displacement(clustering, ds, metric).items()) for metric in ("cosine", "euclidean")}
    print("msd:", {m: [(tau, len(v)) for tau, v in rows][:6] for m, rows in out["msd"].items()})
    out["errors"] = {k: caught(lambda v=v: smooth.find_distribution_peak(v)) for k, v in RS.DEGENERATE.items()}
    out["errors"]["unknown_method"] = caught(lambda: smooth.find_distribution_peak(np.arange(5.0), method="mode"))
    print("errors:", out["errors"])
    path = os.path.join(ROOT, "tests", "golden", "smoothness.pt")
    torch.save(out, path)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
