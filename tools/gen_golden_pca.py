"""Writes tests/golden/pca.pt: what the reference's compute_pca and an identically configured sklearn fit give on the case table of
tests/ref_pca.py.  Needs sklearn and pandas; the tests do not need sklearn: they read the golden.

    python tools/gen_golden_pca.py <reference checkout>/packages/viscy-utils/src/viscy_utils/evaluation/dimensionality_reduction.py

The reference module is loaded by path with ``xarray`` stubbed (it is imported for an isinstance check only).  Results only, no
inputs: the table rebuilds them from seeds.  Per case and per normalize_features ("norm" / "raw"):
  pc_features            the reference's compute_pca(x, n_components, normalize_features)[0], float32 as returned; its first
                         PC_COLUMNS = 16 columns (the tests compare the eight planted components; all 64 columns of the
                         1000-row case alone would be half a megabyte)
  components, explained_variance, ratio, n_components
                         StandardScaler (if normalised) -> PCA(n_components, random_state=42).fit, as the reference configures it
  err_ref                the reference-as-run's distance from the float64 restatement: (variance error relative to the largest
                         variance | max ratio error, max 1 - |cos| over the compared components, max |dZ| / max |Z|)
  gram_err_f32           the same three numbers for the float32 emulation of csrc/pca.hip (tests recompute and compare)
and per case the scaler's mean_, var_, scale_ and the first four standardised rows."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import ref_pca as RP  # noqa: E402

PC_COLUMNS = 16


def load_reference(path):
    stub = types.ModuleType("xarray")
    stub.Dataset = type("Dataset", (), {})
    sys.modules.setdefault("xarray", stub)
    spec = importlib.util.spec_from_file_location("reference_dimensionality_reduction", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    import sklearn
    from sklearn.decomposition import PCA
    from sklearn.preprocessing import StandardScaler

    ref = load_reference(sys.argv[1])
    out = {"cases": {}, "numpy": np.__version__, "sklearn": sklearn.__version__}
    for name, c in RP.CASES.items():
        x = RP.build(name)
        sc = StandardScaler().fit(x)
        entry = {"scaler_mean": torch.from_numpy(sc.mean_.copy()), "scaler_var": torch.from_numpy(sc.var_.copy()),
                 "scaler_scale": torch.from_numpy(sc.scale_.copy()), "scaled_head": torch.from_numpy(sc.transform(x)[:4].copy())}
        for normalize in RP.NORMALIZE:
            pc, df = ref.compute_pca(x, n_components=c["k"], normalize_features=normalize)
            assert pc.dtype == np.float32 and list(df.columns) == [f"PC{i + 1}" for i in range(pc.shape[1])]
            est = PCA(n_components=c["k"], random_state=42).fit(StandardScaler().fit_transform(x) if normalize else x)
            ours = RP.restatement(name, normalize)
            idx = RP.compared(name, normalize)
            lead = [i for i in range(min(RP.PLANTED, c["d"], c["N"] - 1)) if RP.gaps_ok(ours["all_variance"], i)]
            assert c["d"] < 8 or len(lead) == min(RP.PLANTED, c["N"] - 1), (name, normalize, lead, ours["all_variance"][:10])
            assert est.n_components_ == ours["n_components"] == pc.shape[1], (name, est.n_components_, ours["n_components"])
            res = dict(explained_variance=est.explained_variance_, ratio=est.explained_variance_ratio_, components=est.components_, Z=pc)
            err_ref = RP.errors(res, ours, idx)
            emu = RP.gram_err_f32(name, normalize)
            assert RP.signs_agree(est.components_, ours, RP.decided(name, normalize)), (name, normalize)
            print(f"{name:18s} {'norm' if normalize else 'raw ':4s} k {pc.shape[1]:3d} compared {len(idx):2d}  err_ref var {err_ref[0]:.2e} "
                  f"cos {err_ref[1]:.2e} Z {err_ref[2]:.2e}  | emulation var {emu[0]:.2e} cos {emu[1]:.2e} Z {emu[2]:.2e}  "
                  f"solver {est._fit_svd_solver}")
            entry["norm" if normalize else "raw"] = {
                "pc_features": torch.from_numpy(pc[:, :PC_COLUMNS].copy()), "components": torch.from_numpy(est.components_.copy()),
                "explained_variance": torch.from_numpy(est.explained_variance_.copy()),
                "ratio": torch.from_numpy(est.explained_variance_ratio_.copy()), "n_components": int(est.n_components_),
                "err_ref": tuple(float(v) for v in err_ref), "gram_err_f32": tuple(float(v) for v in emu)}
        out["cases"][name] = entry
    path = os.path.join(ROOT, "tests", "golden", "pca.pt")
    torch.save(out, path)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1_000_000


if __name__ == "__main__":
    main()
